// tpx_ci.hip.h — wave-cooperative CSV cell index for LDS-staged csv stages.
//
// Appended after tpx_rt.hip.h to the source of stages that take the index path
// (codegen.StageCodegen.cell_index); every other stage's source is unchanged.
// The scalar per-lane functions are plain C under TPX_HOST_TEST
// (tests/host_cellindex_test.cpp); only the wave glue is device-only.

// ---- wave-cooperative cell index ------------------------------------------------
// While a wave stages its span into LDS it has every byte in registers, 16 B
// per lane per trip, all 64 lanes active. The index classifies those bytes
// there — uniform work — instead of every lane classifying its own row in
// divergent 64-B groups (tpx_mw_group): per 16 bytes five exact 32-bit SWAR
// class masks, quote parity by in-lane prefix-xor + ballot, one packed 32-bit
// wave exscan for the ordinals, and one LDS entry per STRUCTURAL byte (a
// delimiter or '\n' at even quote parity, parity 0 at the wave's first row).
//
// Region layout (TPX_CI_BYTES per wave, 8-aligned):
//   u16 rf[65]   rf[k] = ordinal of the first entry of row k of the batch
//                (rf[0] = 0; 0xFFFF = never written)
//   u64 bad[16]  bit b of word t: 16-B block 64t+b of the span holds a byte
//                >= 0x80, or a '\r' not directly followed by a structural '\n'
//   u32 ent[CAP] {span position : 14, 0 : 1, is '\n' : 1, running count of
//                '"' bytes before it, mod 2^16 : 16}
// A span that ends without '\n' gets one VIRTUAL entry {span, not '\n'} so its
// last row has a terminator entry like any other.
#define TPX_CI_BYTES 4096
#define TPX_CI_RF_OFF 0
#define TPX_CI_BAD_OFF 136
#define TPX_CI_ENT_OFF 264
#define TPX_CI_CAP ((TPX_CI_BYTES - TPX_CI_ENT_OFF) / 4)
#define TPX_CI_NONE 0xFFFFu

// 16-bit positional class masks of a lane's 16 bytes (bit j = byte j), cut to
// `valid`: q '"', s delimiter or '\n', n '\n', r '\r', h byte >= 0x80
struct tpx_ci_cls { unsigned q, s, n, r, h; };

__device__ __forceinline__ void tpx_ci_classify(unsigned w0, unsigned w1,
                                                unsigned w2, unsigned w3,
                                                char delim, unsigned valid,
                                                tpx_ci_cls* c) {
    const unsigned one = 0x01010101u;
    unsigned pq = one * (unsigned)'"', pd = one * (unsigned char)delim;
    unsigned pn = one * (unsigned)'\n', pr = one * (unsigned)'\r';
    unsigned w[4] = {w0, w1, w2, w3};
    unsigned q = 0, s = 0, n = 0, r = 0, h = 0;
    #pragma unroll
    for (int d = 0; d < 4; ++d) {
        unsigned v = w[d];
        unsigned zn = tpx_bs_zero32(v ^ pn);
        q |= tpx_bs_pack4(tpx_bs_zero32(v ^ pq)) << (4 * d);
        s |= tpx_bs_pack4(tpx_bs_zero32(v ^ pd) | zn) << (4 * d);
        n |= tpx_bs_pack4(zn) << (4 * d);
        r |= tpx_bs_pack4(tpx_bs_zero32(v ^ pr)) << (4 * d);
        h |= tpx_bs_pack4(v & 0x80808080u) << (4 * d);
    }
    c->q = q & valid; c->s = s & valid; c->n = n & valid;
    c->r = r & valid; c->h = h & valid;
}

// the in-lane quote state is tpx_bs_inq of tpx_rt.hip.h, which the boundary
// kernels share; the index keeps its own name for it
__device__ __forceinline__ unsigned tpx_ci_inq(unsigned q16, unsigned par) {
    return tpx_bs_inq(q16, par);
}

// one lane's structural bytes -> entries ord0.. in position order; an
// entry past the capacity is dropped (the batch then falls back as a whole)
__device__ __forceinline__ void tpx_ci_scatter(char* ci, int k, unsigned s16,
                                               unsigned n16, unsigned q16,
                                               unsigned ord, unsigned nl,
                                               unsigned qc0) {
    unsigned* ent = (unsigned*)(ci + TPX_CI_ENT_OFF);
    unsigned short* rf = (unsigned short*)(ci + TPX_CI_RF_OFF);
    while (s16) {
        int j = __ffs((int)s16) - 1;
        unsigned isnl = (n16 >> j) & 1u;
        unsigned qc = qc0 + (unsigned)__popc(q16 & ((1u << j) - 1u));
        if (ord < TPX_CI_CAP)
            ent[ord] = (unsigned)(k + j) | (isnl << 15) | (qc << 16);
        ++ord;
        if (isnl) {
            ++nl;
            if (nl <= 64 && ord <= TPX_CI_CAP) rf[nl] = (unsigned short)ord;
        }
        s16 &= s16 - 1;
    }
}

// Row r of the batch occupies span bytes [rs, re); rend is its end after the
// loader's strip of a trailing '\n' and then '\r'. Returns 1 if the row may
// take its cells from the index, 0 if it must be walked by tpx_mw_cell.
//
// Why an accepted row equals tpx_csv_next_cell's walk. The entries
// [rf[r], rf[r+1]) end with the first terminator ('\n' or virtual) after
// entry rf[r]-1, which (r > 0) is required to be the '\n' at rs-1, and the
// terminator is required to sit at re-1 (virtual: at re == span). Entries
// are in position order and every structural byte of the span has one, so
// they are exactly the structural bytes of [rs, re), all delimiters but the
// last, and the parity is 0 at rs. Induction over the cells, with parity 0
// at the cell's start cs and ce the next entry (rend for the last cell):
//  - zero '"' bytes in [cs, ce): parity stays 0, so ce is the FIRST delimiter
//    byte at or after cs; next_cell takes the unquoted branch (no leading
//    quote) and returns p = cs, n = ce - cs, *more = ce < rend. flags 0: no
//    '"' by the count, no '\r' by the bad bitmap (the stripped one is
//    outside), ',' is the delimiter itself.
//  - two '"' bytes, at cs and ce-1: next_cell takes the quoted branch, its
//    first '"' after cs+1 is ce-1, followed by the delimiter or rend, so no
//    escape and no junk: p = cs+1, n = ce-cs-2, flags 1|8, and the scan for
//    the delimiter from ce finds it at once. Commas and newlines inside were
//    at odd parity and never became entries.
//  Both leave parity 0 at ce+1. With exactly ncols entries `avail` is true
//  before each cell and false after the last, so neither UNDERRUN nor
//  OVERRUN; no flag has bit 2 or 4; and no byte of [rs, re) is >= 0x80 by
//  the bitmap, which is what the walk's ASCII gate reports for a fully
//  walked row. Anything else — other quote counts or places, a shared block
//  with a neighbour's high byte, CR in content, a wrong cell count, offsets
//  that are not the even-parity newlines — declines; a declined row is
//  walked from its start, so results never depend on this function being
//  right about an odd row, only on it saying no.
__device__ __forceinline__ int tpx_ci_row(const char* base, const char* ci,
                                          int r, int rs, int re, int rend,
                                          int span, int ncols, int* e0_out) {
    const unsigned* ent = (const unsigned*)(ci + TPX_CI_ENT_OFF);
    const unsigned short* rf = (const unsigned short*)(ci + TPX_CI_RF_OFF);
    const unsigned long long* bad =
        (const unsigned long long*)(ci + TPX_CI_BAD_OFF);
    if (re <= rs) return 0;
    unsigned e0 = rf[r], e1 = rf[r + 1];
    if (e0 == TPX_CI_NONE || e1 == TPX_CI_NONE) return 0;
    if (e1 != e0 + (unsigned)ncols) return 0;
    unsigned q = 0;
    if (e0 == 0) {
        if (r != 0) return 0;
    } else {
        unsigned pe = ent[e0 - 1];
        if (!(pe & 0x8000u) || (int)(pe & 0x3FFFu) != rs - 1) return 0;
        q = pe >> 16;
    }
    unsigned le = ent[e1 - 1];
    int lp = (int)(le & 0x3FFFu);
    if (le & 0x8000u) {
        if (lp != re - 1) return 0;
    } else {  // virtual terminator: the last row of the input has no '\n'
        if (lp != re || re != span) return 0;
    }
    int b0 = rs >> 4, b1 = (re - 1) >> 4;
    for (int w = b0 >> 6; w <= (b1 >> 6); ++w) {
        int lo = w == (b0 >> 6) ? (b0 & 63) : 0;
        int hi = w == (b1 >> 6) ? (b1 & 63) : 63;
        unsigned long long m = (~0ULL << lo) & (~0ULL >> (63 - hi));
        if (bad[w] & m) return 0;
    }
    int cs = rs;
    for (int k = 0; k < ncols; ++k) {
        unsigned e = ent[e0 + (unsigned)k];
        int ce = k == ncols - 1 ? rend : (int)(e & 0x3FFFu);
        unsigned nq = ((e >> 16) - q) & 0xFFFFu;
        if (nq && (nq != 2 || ce - cs < 2 || base[cs] != '"' ||
                   base[ce - 1] != '"'))
            return 0;
        q = e >> 16;
        cs = (int)(e & 0x3FFFu) + 1;
    }
    *e0_out = (int)e0;
    return 1;
}

// cell k of a row that tpx_ci_row accepted
__device__ __forceinline__ void tpx_ci_cell(const char* base, const char* ci,
                                            int e0, int k, int ncols, int rs,
                                            int rend, tpx_cell* c) {
    const unsigned* ent = (const unsigned*)(ci + TPX_CI_ENT_OFF);
    unsigned e = ent[e0 + k];
    int cs = rs;
    unsigned q = 0;
    if (e0 + k > 0) {
        unsigned pe = ent[e0 + k - 1];
        cs = (int)(pe & 0x3FFFu) + 1;
        q = pe >> 16;
    }
    int ce = k == ncols - 1 ? rend : (int)(e & 0x3FFFu);
    if (((e >> 16) - q) & 0xFFFFu) {
        c->p = base + cs + 1; c->n = ce - cs - 2; c->flags = 1 | 8;
    } else {
        c->p = base + cs; c->n = ce - cs; c->flags = 0;
    }
}

#ifndef TPX_HOST_TEST  // device-only: the wave glue of the index builder
// Stage span bytes [0, span) of the wave's batch from global memory into
// wave_lds, as the plain staging loop does, and build the cell index of the
// bytes from `lo` (the first row's start; the span start is rounded down to
// 16) in `ci`. Called by all 64 lanes. Returns false, the same in every
// lane, if the entries did not fit: the batch then uses the walk.
__device__ __forceinline__ bool tpx_ci_stage(char* wave_lds, char* ci,
                                             const char* src, int span, int lo,
                                             char delim, int lane) {
    unsigned* ent = (unsigned*)(ci + TPX_CI_ENT_OFF);
    unsigned short* rf = (unsigned short*)(ci + TPX_CI_RF_OFF);
    unsigned long long* bad = (unsigned long long*)(ci + TPX_CI_BAD_OFF);
    rf[lane + 1] = (unsigned short)TPX_CI_NONE;
    if (lane == 0) rf[0] = 0;
    // wave-uniform carries between trips
    unsigned car_ord = 0, car_nl = 0, car_q = 0;
    bool pend = false;  // lane 63's last byte was a '\r': the next byte decides
    unsigned long long below = (1ull << lane) - 1ull;
    int trip = 0;
    // the next trip's 16 bytes are loaded before this trip's are classified,
    // so the global-load latency overlaps the ALU work instead of adding up
    uint4 pre = make_uint4(0, 0, 0, 0);
    if (lane * 16 + 16 <= span) pre = *(const uint4*)(src + lane * 16);
    for (int kb = 0; kb < span; kb += 64 * 16, ++trip) {
        int k = kb + lane * 16;
        unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        if (k + 16 <= span) {
            uint4 v = pre;
            if (k + 64 * 16 + 16 <= span)
                pre = *(const uint4*)(src + k + 64 * 16);
            *(uint4*)(wave_lds + k) = v;
            w0 = v.x; w1 = v.y; w2 = v.z; w3 = v.w;
        } else {
            unsigned long long a = 0, b = 0;
            for (int j = k; j < span; ++j) {
                unsigned char ch = (unsigned char)src[j];
                wave_lds[j] = (char)ch;
                int t = j - k;
                if (t < 8) a |= (unsigned long long)ch << (8 * t);
                else b |= (unsigned long long)ch << (8 * (t - 8));
            }
            w0 = (unsigned)a; w1 = (unsigned)(a >> 32);
            w2 = (unsigned)b; w3 = (unsigned)(b >> 32);
        }
        int nv = span - k; nv = nv < 0 ? 0 : (nv > 16 ? 16 : nv);
        int nl_ = lo - k; nl_ = nl_ < 0 ? 0 : (nl_ > 16 ? 16 : nl_);
        unsigned valid = ((1u << nv) - 1u) & ~((1u << nl_) - 1u);
        tpx_ci_cls c;
        tpx_ci_classify(w0, w1, w2, w3, delim, valid, &c);
        unsigned pq = (unsigned)__popc(c.q);
        unsigned long long oddm = __ballot(pq & 1u);
        unsigned par = (car_q ^ (unsigned)__popcll(oddm & below)) & 1u;
        unsigned inq = tpx_ci_inq(c.q, par);
        unsigned s16 = c.s & ~inq, n16 = c.n & ~inq;
        // fields of 11/11/10 bits: an exclusive prefix is at most 63*16
        unsigned ps = (unsigned)__popc(s16), pn = (unsigned)__popc(n16);
        unsigned ex = tpx_wave_exscan32(ps | (pn << 11) | (pq << 22), lane);
        unsigned xs = ex & 0x7FFu, xn = (ex >> 11) & 0x7FFu, xq = ex >> 22;
        // '\r' followed by anything but a structural '\n'
        unsigned long long nlf = __ballot(n16 & 1u);
        unsigned nxt = lane < 63 ? (unsigned)((nlf >> (lane + 1)) & 1ull) : 0u;
        unsigned badr = c.r & ~((n16 >> 1) | (nxt << 15));
        bool mypend = lane == 63 && (badr & 0x8000u);
        if (lane == 63) badr &= 0x7FFFu;
        unsigned long long bw = __ballot(c.h != 0 || badr != 0);
        if (lane == 0) {
            if (pend && !(nlf & 1ull)) bad[trip - 1] |= 1ull << 63;
            bad[trip] = bw;
        }
        pend = __ballot(mypend) != 0;
        tpx_ci_scatter(ci, k, s16, n16, c.q, car_ord + xs, car_nl + xn,
                       car_q + xq);
        car_ord += (unsigned)__builtin_amdgcn_readlane((int)(xs + ps), 63);
        car_nl += (unsigned)__builtin_amdgcn_readlane((int)(xn + pn), 63);
        car_q += (unsigned)__builtin_amdgcn_readlane((int)(xq + pq), 63);
    }
    if (pend && lane == 0) bad[trip - 1] |= 1ull << 63;
    bool ok = car_ord < TPX_CI_CAP;
    if (ok && car_nl < 64 && lane == 0) {
        ent[car_ord] = (unsigned)span | (car_q << 16);
        rf[car_nl + 1] = (unsigned short)(car_ord + 1);
    }
    __builtin_amdgcn_wave_barrier();
    return ok;
}
#endif  // TPX_HOST_TEST
