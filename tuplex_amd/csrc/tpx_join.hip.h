// tpx_join.hip.h — hash-join build tables that live in HBM (device join table).
//
// Appended after tpx_rt.hip.h only by stages whose join probes a device table
// (codegen._jt_section), the way tpx_re.hip.h / tpx_ci.hip.h are; every other
// stage's source is unchanged. The build side (unique, non-null keys) is
// uploaded once as Arrow-layout columns — exactly the 3-pointers-per-column
// slot convention of tpx_stage_execute_col / tpx_table — and a slot table is
// built over it by tpx_join_build_i64 / tpx_join_build_str (one thread per
// build row). The generated stage declares `__device__ TpxJoinTab tpx_jt[NJ]`;
// the library fills entry i before a run (tpx_stage_bind_jtable), so the
// source depends on the build side's schema only, never on its contents.
//
// Slot layout, and why. A probe is one dependent random read per step, and a
// table that has left the Infinity Cache pays a full HBM miss for each one
// (MI355X_MICROARCH.md, Infinity Cache / Indexed rows), so a step must touch
// one cache line and decide there in the common case:
//  - i64 key: 16-byte slots {key, row}, 16-byte aligned, so a slot never
//    straddles a line and hit, miss-on-empty and collision are all decided
//    from one 16-byte load. Four slots share a 64-byte line, so a short probe
//    run usually stays in the line it started in.
//  - str key: 8-byte slots {row (low 32), upper 32 hash bits (high 32)}. A
//    colliding slot is rejected on the hash bits without touching string
//    bytes; only a slot whose 32 bits agree (the hit, or one in 2^32) reads
//    the key column's offsets and bytes. Eight slots per 64-byte line.
// "Empty" is row == -1 (the table is memset to 0xFF), never a key value:
// every int64, 0 and -1 included, is a legal key.
//
// Build: keys are known unique (the plan checks), so an insert never compares
// keys, it only claims the first free slot from its home with atomicCAS.
// The i64 insert claims the row field and then stores the key (same thread);
// the str insert publishes the whole 8-byte slot with one 64-bit CAS. Probes
// run only in later launches, so neither needs a fence. The table has
// tsize >= 2 n slots (smallest power of two, at least 8 — the rule of the
// embedded table), so a free slot always exists.
//
// The per-row pieces are plain C under TPX_HOST_TEST
// (tests/host_join_test.cpp); only the __global__ wrappers are device-only.

#define TPX_JOIN_MAX_COLS 64

struct TpxJoinSlotI {   // i64-key slot
    long long key;
    int row;            // build row, -1 = empty
    int pad;
};

struct TpxJoinTab {
    void* slots;                 // TpxJoinSlotI[mask+1] or u64[mask+1]
    unsigned long long mask;     // tsize - 1
    long long n_rows;            // build rows
    int n_cols;                  // build columns
    int key_col;                 // which of them is the key
    // 3 device pointers per build column (tpx_stage_execute_col layout):
    // [3j] values (8 B; bool 1 B) or int64 offsets (n_rows+1) of a string
    // column, [3j+1] string bytes, [3j+2] null mask (uint8, 1 = null) or 0
    const void* cols[3 * TPX_JOIN_MAX_COLS];
};

#define TPX_JOIN_EMPTY64 0xFFFFFFFFFFFFFFFFULL

// claim the first free slot from the key's home; returns the slot, or -1 if
// the table is full (cannot happen with tsize >= 2 n)
__device__ __forceinline__ long long tpx_join_insert_i64(
        TpxJoinSlotI* slots, unsigned long long mask, long long key, int row) {
    unsigned long long h = tpx_hash_i64(key);
    for (unsigned long long p = 0; p <= mask; ++p) {
        unsigned long long s = (h + p) & mask;
        if (atomicCAS(&slots[s].row, -1, row) == -1) {
            slots[s].key = key;
            return (long long)s;
        }
    }
    return -1;
}

__device__ __forceinline__ long long tpx_join_insert_str(
        unsigned long long* slots, unsigned long long mask,
        const char* p, long long n, int row) {
    unsigned long long h = tpx_jhash_bytes(p, n);
    unsigned long long word = (h & 0xFFFFFFFF00000000ULL) |
                              (unsigned long long)(unsigned)row;
    for (unsigned long long q = 0; q <= mask; ++q) {
        unsigned long long s = (h + q) & mask;
        if (atomicCAS(&slots[s], TPX_JOIN_EMPTY64, word) == TPX_JOIN_EMPTY64)
            return (long long)s;
    }
    return -1;
}

// build row of `key`, or -1. Ends at an empty slot or after mask+1 steps.
__device__ __forceinline__ int tpx_join_probe_i64(const TpxJoinTab& t,
                                                  long long key) {
    const TpxJoinSlotI* slots = (const TpxJoinSlotI*)t.slots;
    unsigned long long h = tpx_hash_i64(key);
    for (unsigned long long p = 0; p <= t.mask; ++p) {
        TpxJoinSlotI s = slots[(h + p) & t.mask];
        if (s.row < 0) return -1;
        if (s.key == key) return s.row;
    }
    return -1;
}

// string equality is length plus bytes, like the embedded probe
__device__ __forceinline__ int tpx_join_probe_str(const TpxJoinTab& t,
                                                  tstr key) {
    const unsigned long long* slots = (const unsigned long long*)t.slots;
    const long long* offs = (const long long*)t.cols[3 * t.key_col];
    const char* bytes = (const char*)t.cols[3 * t.key_col + 1];
    unsigned long long h = tpx_jhash_bytes(key.p, key.n);
    unsigned hi = (unsigned)(h >> 32);
    for (unsigned long long p = 0; p <= t.mask; ++p) {
        unsigned long long w = slots[(h + p) & t.mask];
        int row = (int)(unsigned)w;
        if (row < 0) return -1;
        if ((unsigned)(w >> 32) != hi) continue;
        long long o = offs[row];
        if (tpx_streq(tstr{bytes + o, offs[row + 1] - o}, key)) return row;
    }
    return -1;
}

#ifndef TPX_HOST_TEST
// one thread per build row (grid-stride); slots were memset to 0xFF
extern "C" __global__ void tpx_join_build_i64(
        const long long* __restrict__ keys, long long n, TpxJoinSlotI* slots,
        unsigned long long mask) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride)
        tpx_join_insert_i64(slots, mask, keys[i], (int)i);
}

extern "C" __global__ void tpx_join_build_str(
        const long long* __restrict__ offs, const char* __restrict__ bytes,
        long long n, unsigned long long* slots, unsigned long long mask) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        long long o = offs[i];
        tpx_join_insert_str(slots, mask, bytes + o, offs[i + 1] - o, (int)i);
    }
}
#endif  // TPX_HOST_TEST
