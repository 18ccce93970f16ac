// tpx_cache.hip.h — device pack of a stage's kept rows into dense Arrow-layout
// columns (cache() partitions that stay in HBM).
//
// Appended after tpx_rt.hip.h by codegen.runtime_header(). Before the write
// kernel a stage's output is columnar but sparse: per output column the outv
// slots [8-byte value or string pointer, 4-byte string length, 1-byte null
// flag], one entry per INPUT row, plus keep[] and its exclusive scan (the
// rank). These fixed kernels compact that into exactly what the columnar
// source (codegen._load_inputs_col) reads: 8-byte value arrays, 1-byte bool
// arrays, int64 offsets (m+1) + one contiguous data buffer per string column,
// uint8 null masks, and int64 row keys. The executor (csrc/tpx_abi.cpp,
// pack_table) owns the order: tpx_cache_pack_fixed, one tpx_scan_block
// exclusive scan per string column, tpx_cache_gather_str.
//
// The per-lane pieces are plain C under TPX_HOST_TEST
// (tests/host_cachepack_test.cpp); only the wave glue is device-only.

// what one descriptor of tpx_cache_pack_fixed moves for a kept row
#define TPX_CP_VAL8 0  // 8-byte value (i64 / f64 bits)           -> 8 bytes
#define TPX_CP_BOOL 1  // 8-byte slot holding 0 / 1               -> 1 byte
#define TPX_CP_MASK 2  // 1-byte null flag                        -> 1 byte
#define TPX_CP_LEN 3   // 4-byte string length, 0 where null      -> int64

struct tpx_cp_desc {
    const void* src;           // outv slot, indexed by input row
    void* dst;                 // dense array, indexed by rank
    const unsigned char* nul;  // TPX_CP_LEN: the column's null flags, or 0
    long long kind;
};

// bytes a row contributes to its string column: none where null; a negative
// length (never produced by a stage) counts as empty in BOTH kernels
__device__ __forceinline__ long long tpx_cp_len(int len, bool is_null) {
    return (is_null || len < 0) ? 0 : (long long)len;
}

// move input row i of one descriptor to dense position r
__device__ __forceinline__ void tpx_cp_move(const tpx_cp_desc& d, long long i,
                                            long long r) {
    switch (d.kind) {
    case TPX_CP_VAL8:
        ((unsigned long long*)d.dst)[r] = ((const unsigned long long*)d.src)[i];
        break;
    case TPX_CP_BOOL:
        ((unsigned char*)d.dst)[r] = ((const long long*)d.src)[i] != 0 ? 1 : 0;
        break;
    case TPX_CP_MASK:
        ((unsigned char*)d.dst)[r] = ((const unsigned char*)d.src)[i] ? 1 : 0;
        break;
    default:  // TPX_CP_LEN
        ((long long*)d.dst)[r] =
            tpx_cp_len(((const int*)d.src)[i], d.nul && d.nul[i]);
        break;
    }
}

// Which of 64 rows owns destination byte j: the number of rows whose
// inclusive length prefix incl(k) is <= j (incl non-decreasing, incl(63) > j;
// rows of length 0 own nothing and are stepped over). Six probes, of rows
// 0..62 only. `incl` is a lane shuffle on the device, an array in the host test.
template <class F>
__device__ __forceinline__ int tpx_cp_owner(F incl, unsigned j) {
    int lo = 0;
    #pragma unroll
    for (int s = 32; s; s >>= 1)
        if (incl(lo + s - 1) <= j) lo += s;
    return lo;
}

#ifndef TPX_HOST_TEST
// One launch packs every fixed-width column, null mask, string length and the
// row keys: grid-stride over input rows, a kept row i lands at rank[i]. Ranks
// of neighbouring kept rows are neighbours, so the stores of a wave fall into
// one or two runs per array.
extern "C" __global__ void tpx_cache_pack_fixed(
    const unsigned char* __restrict__ keep, const long long* __restrict__ rank,
    long long n, long long row0, const tpx_cp_desc* __restrict__ desc,
    int ndesc, long long* __restrict__ rowkey) {
    long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        if (!keep[i]) continue;
        long long r = rank[i];
        rowkey[r] = row0 + i;
        for (int k = 0; k < ndesc; ++k) tpx_cp_move(desc[k], i, r);
    }
}

// String gather: one wave per 64-row batch, grid-stride. The kept rows of a
// batch are neighbours in the destination — bytes [offs[rank[first row]],
// + batch total) — so the copy is driven from the DESTINATION: each trip the
// wave owns 64 consecutive destination bytes, every lane finds the row its
// byte belongs to by a six-step search over the wave's length prefixes
// (tpx_cp_owner through lane shuffles) and fetches that one byte from the
// row's source. Stores are one coalesced 64-byte run per trip whatever the
// cell lengths, all lanes stay busy on short cells, and sources (input bytes
// or the string heap, any alignment) are only ever read bytewise. No byte
// outside the batch's destination range is written. A batch of 4 GiB or more
// (prefixes past 32 bits) is copied row by row instead.
extern "C" __global__ void tpx_cache_gather_str(
    const unsigned char* __restrict__ keep, const long long* __restrict__ rank,
    long long n, const unsigned long long* __restrict__ sptr,
    const int* __restrict__ slen, const unsigned char* __restrict__ snull,
    const long long* __restrict__ offs, char* __restrict__ data) {
    int lane = threadIdx.x & 63;
    long long nb = (n + 63) >> 6;
    long long wave_stride = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long wb = (long long)blockIdx.x * (blockDim.x >> 6) +
                        (threadIdx.x >> 6);
         wb < nb; wb += wave_stride) {
        long long r = wb * 64 + lane;
        bool kept = r < n && keep[r];
        long long len = kept ? tpx_cp_len(slen[r], snull && snull[r]) : 0;
        unsigned long long src = len ? sptr[r] : 0ull;
        long long before = tpx_wave_exscan(len);
        long long total = __shfl(before + len, 63);
        if (total == 0) continue;  // wave-uniform
        char* dst = data + offs[rank[wb * 64]];
        if (total < (1ll << 32)) {
            unsigned incl = (unsigned)(before + len);
            unsigned excl = (unsigned)before;
            unsigned lo32 = (unsigned)src, hi32 = (unsigned)(src >> 32);
            // uniform trip count: the shuffles need every lane
            for (long long base = 0; base < total; base += 64) {
                long long j = base + lane;
                bool live = j < total;
                unsigned jj = (unsigned)(live ? j : total - 1);
                int o = tpx_cp_owner(
                    [&](int k) { return (unsigned)__shfl(incl, k); }, jj);
                unsigned e = __shfl(excl, o);
                unsigned long long p =
                    (unsigned long long)__shfl(lo32, o) |
                    ((unsigned long long)__shfl(hi32, o) << 32);
                if (live) dst[j] = ((const char*)p)[jj - e];
            }
        } else {
            for (int k = 0; k < 64; ++k) {
                long long lk = __shfl(len, k);
                long long bk = __shfl(before, k);
                const char* pk = (const char*)(
                    (unsigned long long)__shfl((unsigned)src, k) |
                    ((unsigned long long)__shfl((unsigned)(src >> 32), k)
                     << 32));
                for (long long b = lane; b < lk; b += 64) dst[bk + b] = pk[b];
            }
        }
    }
}
#endif  // TPX_HOST_TEST
