/* tpx_abi.h — C-ABI drop-in boundary of the MI355X-native TransformStage executor.
 *
 * This is the replacement for the reference's JITSymbols contract: Tuplex's
 * LocalBackend resolves per-stage function pointers by name from its LLVM JIT
 * (reference: tuplex/core/include/physical/TransformStage.h:291-314, resolved in
 * TransformStage.cc:763-846; functor signatures tuplex/core/include/CodeDefs.h:48,
 * :55, :94-116) and hands each executor thread a `read_block_f` to run over raw
 * partition bytes (TransformTask.cc:382 execute). Here the whole per-stage surface is
 * collapsed into: compile a stage (tpx_stage_compile — replaces TransformStage::compile
 * TransformStage.cc:763) and execute it over a partition batch (tpx_stage_execute —
 * replaces LocalBackend::executeTransformStage LocalBackend.cc:815 +
 * TransformTask.cc:682 processMemorySource / :724 processFileSource).
 *
 * Byte formats crossing this boundary are the reference's:
 *  - partitions: [int64 numRows][rows...] (Partition.h:38), rows in the Tungsten-style
 *    layout of utils/src/Serializer.cc:20-24 (+:29 bitmap, :1097 varlen info word);
 *  - exception buffers: records [row,ec,opID,size][data] per
 *    core/include/physical/IExceptionableTask.h:20 serializeExceptionToMemory;
 *  - error codes: ExceptionCodes.h:26 (SUCCESS=0).
 * So the host resolve/merge path (ResolveTask semantics) runs unchanged on what this
 * library returns.
 *
 * All entry points are extern "C", plain pointers + sizes; no torch types.
 */
#ifndef TPX_ABI_H
#define TPX_ABI_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library / device management ------------------------------------------------ */

/* ABI version (major<<16 | minor). */
int64_t tpx_version(void);

/* Number of visible HIP devices; 0 if none / HIP unavailable. Never throws. */
int64_t tpx_device_count(void);

/* Select device for subsequent calls on this thread (default 0). Returns 0 on
 * success, nonzero HIP error otherwise. */
int64_t tpx_set_device(int64_t device);

/* Last error message (thread-local, NUL-terminated, owned by the library). */
const char* tpx_last_error(void);

/* ---- stage compile (replaces TransformStage::compile, TransformStage.cc:763) ---- */

/* Opaque compiled-stage handle (the analog of JITSymbols, TransformStage.h:291). */
typedef struct tpx_stage tpx_stage;

/* Compile a stage from generated HIP source. `hip_source` is the fused-pipeline
 * kernel source emitted by the front end (the replacement for StageBuilder.cc:602
 * generateFastCodePath's LLVM module); it defines the fixed-name kernels
 * tpx_stage_main / tpx_stage_write plus the runtime's scan kernels. `stage_desc`
 * is a small key=value text descriptor (source/sink kind, in/out column types)
 * the executor uses to size buffers. `cache_dir` (may be NULL) holds hsaco code
 * objects keyed by source hash — the analog of the JIT cache. `flags` bit 0:
 * compile-only (do not load a module; valid on a machine with no GPU).
 * Returns NULL on failure (see tpx_last_error). */
tpx_stage* tpx_stage_compile(const char* hip_source,
                             const char* stage_desc,
                             const char* cache_dir,
                             int64_t flags);

void tpx_stage_free(tpx_stage* stage);

/* ---- stage execute (replaces LocalBackend.cc:815 executeTransformStage) --------- */

/* One input partition: raw bytes in the reference layout ([int64 numRows][rows...])
 * plus the per-row offsets (offsets[i] = byte offset of row i from `data`;
 * offsets[num_rows] = size). Offsets are host-side metadata our PartitionWriter
 * tracks; the reference walks rows serially instead (TransformTask.cc:682). */
typedef struct {
    const uint8_t* data;
    int64_t        size;
    int64_t        num_rows;
    const int64_t* row_offsets;   /* num_rows+1 entries */
} tpx_partition;

/* Execution result. Buffers are allocated by the library; free with
 * tpx_result_free. */
typedef struct {
    /* normal-case output partition, reference layout [int64 numRows][rows...]
     * (csv sink: raw CSV text and out_row_offsets are text offsets) */
    uint8_t* out_data;
    int64_t  out_size;
    int64_t  out_num_rows;
    int64_t* out_row_offsets;     /* out_num_rows+1 entries */
    /* global input row index of each output row (order-merge support; the
     * reference keeps row order via task ordering + ResolveTask.cc:878) */
    int64_t* out_row_indices;     /* out_num_rows entries */
    /* exception buffer: packed records [row,ec,opID,size][data]
     * (IExceptionableTask.h:20); `row` is the global input row index. */
    uint8_t* exc_data;
    int64_t  exc_size;
    int64_t  exc_num_rows;
    /* metrics (JobMetrics.h:23 analog) */
    double   t_h2d_ms, t_kernel_ms, t_d2h_ms;
    int64_t  bytes_in, bytes_out;
    /* per-phase kernel timings (HIP events on the launch stream) */
    double   t_boundary_ms;   /* csv row-boundary scan kernels */
    double   t_main_ms;       /* fused parse+UDF stage kernel (dominant) */
    double   t_compact_ms;    /* prefix-sum compaction (fused csv sink: the
                                 scan over the per-batch descriptors) */
    double   t_write_ms;      /* serialize / csv-format kernel (fused csv
                                 sink: tpx_csv_gather) */
    int64_t  in_num_rows;     /* input rows seen by the stage */
} tpx_result;

/* Run the compiled stage over a batch of memory partitions (mem2mem source,
 * TransformTask.cc:682 processMemorySource analog). Row indices in exception records
 * are global across the batch in input order. Returns 0 on success. */
int64_t tpx_stage_execute(tpx_stage* stage,
                          const tpx_partition* parts, int64_t n_parts,
                          tpx_result* result);

/* Run the compiled stage over raw CSV bytes (file source,
 * TransformTask.cc:724 processFileSource + CSVReader.cc:390 analog). The chunk must
 * start at a row start and end at a row end (host chunker guarantees this, mirroring
 * utils/src/CSVUtils.cc:1494 findLineStart). `csv_desc` is the serialized CSV schema
 * descriptor produced by the front end (delimiter, quote, columns, null values,
 * projected columns, per-column types). If the stage sinks to a file
 * (tocsv), result->out_data holds CSV text bytes and out_row_offsets is NULL. */
int64_t tpx_stage_execute_csv(tpx_stage* stage,
                              const uint8_t* csv_bytes, int64_t size,
                              int64_t first_global_row,
                              tpx_result* result);

void tpx_result_free(tpx_result* result);

/* ---- device-resident input (benchmark / cache() support) ----------------------
 * The reference's partitions live in RAM; ours live in HBM. These let a caller
 * keep input bytes resident across executions (the timed region of bench.py
 * starts with inputs already in HBM; PCIe-inclusive rates are reported
 * separately — DESIGN.md). */
uint64_t tpx_dev_alloc(int64_t size);               /* returns device VA or 0 */
int64_t  tpx_dev_upload(uint64_t dst, const void* src, int64_t size);
void     tpx_dev_free(uint64_t ptr);

/* Pinned host staging for streamed ingestion (file -> pinned ring -> DMA,
 * the read-buffer role of CSVReader.cc:390). Host pointer as u64, 0 on
 * failure. */
uint64_t tpx_pinned_alloc(int64_t size);
void     tpx_pinned_free(uint64_t ptr);

/* Execute over CSV bytes already resident on device. `flags` bit1 (value 2):
 * leave output partitions on device (report sizes/counts only — the device
 * partition manager analog of memory-sink partitions, Partition.h:38). */
int64_t tpx_stage_execute_csv_dev(tpx_stage* stage,
                                  uint64_t dev_bytes, int64_t size,
                                  int64_t first_global_row, int64_t flags,
                                  tpx_result* result);

/* Execute over a COLUMNAR (Arrow-layout) input already resident on device —
 * the ORC ingest path (reference: io/src/OrcTypes.cc + physical OrcReader;
 * SURVEY.md §8f-2). `slots` holds 3 device pointers per input column:
 *   [3k+0] i64/f64 value array (stride 8), bool array (stride 1), or for
 *          strings the int64 offsets array (n_rows+1 entries);
 *   [3k+1] string data base pointer (strings only, else NULL);
 *   [3k+2] null mask (uint8, 1 = null; optional columns only, else NULL).
 * Unused (projection-pushed-down) columns may pass NULL slots. Exception
 * payloads are empty (no row bytes exist); the caller replays exception rows
 * from its own copy of the table by row index. */
int64_t tpx_stage_execute_col(tpx_stage* stage, void* const* slots,
                              int64_t n_slots, int64_t n_rows,
                              int64_t in_bytes, int64_t first_global_row,
                              int64_t flags, tpx_result* result);

/* ---- device-resident cache() partitions ------------------------------------------
 * A tpx_table is one dense columnar (Arrow-layout) partition in HBM that the
 * library owns: the kept rows of one stage execute, packed on the device into
 * exactly the slots tpx_stage_execute_col reads. Its memory is its own
 * (hipMalloc), not workspace-arena memory, so it outlives later executes; it
 * lives on the device that was current when it was made, and every call
 * below selects that device for its own duration. */
typedef struct tpx_table tpx_table;

/* Return code of the cache executes when the table's memory cannot be had
 * (hipMalloc failed, or the byte cap of the TPX_TABLE_MAX_BYTES environment
 * variable — read once — was exceeded). No table is returned, never a partial
 * one; the caller falls back to a host cache. */
#define TPX_E_TABLE_ALLOC 2

/* Cache-mode executes over host / device-resident CSV bytes: the stage runs
 * as in tpx_stage_execute_csv(_dev), but instead of serializing kept rows
 * and copying them out, the pack kernels leave them in *table. The stage
 * must have a mem sink, no aggregate and no fused csv sink. Of the normal
 * output only result->out_num_rows and result->out_row_indices (the global
 * input row index of each table row, 8 bytes per row) are filled; out_data
 * and out_row_offsets stay NULL. Exceptions are returned exactly as by the
 * plain executes. *table is NULL when the input holds no rows. */
int64_t tpx_stage_cache_csv(tpx_stage* stage,
                            const uint8_t* csv_bytes, int64_t size,
                            int64_t first_global_row,
                            tpx_result* result, tpx_table** table);
int64_t tpx_stage_cache_csv_dev(tpx_stage* stage,
                                uint64_t dev_bytes, int64_t size,
                                int64_t first_global_row,
                                tpx_result* result, tpx_table** table);

/* Rows / device bytes of a table; -1 for NULL. */
int64_t tpx_table_rows(const tpx_table* table);
int64_t tpx_table_bytes(const tpx_table* table);

/* Fill `slots` with the table's 3 device pointers per column, in the layout
 * tpx_stage_execute_col takes, and (if non-NULL) `slot_bytes` with the bytes
 * each holds (0 for a NULL slot). Returns 3 * ncols, or -1 if n_slots is
 * smaller than that or table is NULL. */
int64_t tpx_table_slots(const tpx_table* table, void** slots,
                        int64_t* slot_bytes, int64_t n_slots);

/* Copy the columns to host buffers (lazy materialisation): host_slots[k]
 * receives slot k's bytes (tpx_table_slots' slot_bytes[k]); NULL entries are
 * skipped. Returns 0 on success. */
int64_t tpx_table_download(const tpx_table* table, void* const* host_slots,
                           int64_t n_slots);

void tpx_table_free(tpx_table* table);

/* ---- device join tables ----------------------------------------------------------
 * A tpx_jtable is the build side of a unique-key hash join kept in HBM: the
 * build columns as Arrow-layout arrays plus a slot table built over them by
 * the stage module's build kernel (csrc/tpx_join.hip.h). Like a tpx_table it
 * owns its memory (hipMalloc, not workspace-arena memory), lives on the
 * device that was current when it was made and honours TPX_TABLE_MAX_BYTES.
 * A stage whose generated source declares `tpx_jt[]` probes the table that
 * was last bound to the entry; stage handles are shared between pipelines
 * with the same source, so a caller binds immediately before each run. */
typedef struct tpx_jtable tpx_jtable;

/* Upload n_cols build columns of n_rows rows and build the slot table over
 * column key_col (int64 keys, or strings if key_is_str). host_slots holds 3
 * HOST pointers per column in the tpx_stage_execute_col slot layout (values
 * or int64 offsets [n_rows+1] | string bytes | uint8 null mask) and
 * slot_bytes the bytes behind each; a NULL pointer means the slot is absent,
 * a non-NULL one with 0 bytes a present, empty array. Keys must be unique
 * and non-null; at most 64 columns and 2^30 rows. `stage` must be a loaded
 * stage whose source includes the join header. Complete (synchronised) on
 * return. Returns 0; TPX_E_TABLE_ALLOC (and no table, never a partial one)
 * when the memory cannot be had; -1 on any other error. n_rows == 0 gives a
 * valid table on which every probe misses. */
int64_t tpx_jtable_build(tpx_stage* stage, void* const* host_slots,
                         const int64_t* slot_bytes, int64_t n_cols,
                         int64_t n_rows, int64_t key_col, int64_t key_is_str,
                         tpx_jtable** out);

/* Make `table` the one the stage's join_index-th device join probes, for
 * every execute entry point, until the next bind of that entry. */
int64_t tpx_stage_bind_jtable(tpx_stage* stage, int64_t join_index,
                              const tpx_jtable* table);

/* Build rows / device bytes (-1 for NULL); HIP-event time of the build
 * kernel in ms (0 for an empty build side, -1 for NULL). */
int64_t tpx_jtable_rows(const tpx_jtable* table);
int64_t tpx_jtable_bytes(const tpx_jtable* table);
double  tpx_jtable_build_ms(const tpx_jtable* table);

void tpx_jtable_free(tpx_jtable* table);

/* Cumulative per-process byte counts of the host<->device copies the library
 * has issued (device-to-device copies count as neither). Either pointer may
 * be NULL. Works without a GPU. Returns 0. */
int64_t tpx_xfer_stats(int64_t* h2d_bytes, int64_t* d2h_bytes);

/* Generated-source introspection (debug / judge). Returns the HIP source the stage
 * was compiled from (owned by the stage). */
const char* tpx_stage_source(const tpx_stage* stage);

#ifdef __cplusplus
}
#endif
#endif /* TPX_ABI_H */
