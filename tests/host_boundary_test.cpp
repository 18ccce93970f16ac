// Host-compiled check of the CSV boundary kernels (csrc/tpx_rt.hip.h):
// tpx_csv_chunk_stats and tpx_csv_emit_rows are replayed with their 64 lanes
// and four trips emulated one after another. The wave glue (ballot, bit counts
// below a lane, sums, ranks) is plain C here; everything a lane does to its 16
// bytes goes through the very per-lane functions the kernels call
// (tpx_bs_detect, tpx_bs_count16, tpx_bs_rows16, tpx_bs_load_tail). q / c0 /
// c1 per chunk and the emitted offsets are compared with a byte-serial state
// machine. The input sits at the end of an exact-size heap block, so a read at
// or after `size` is an error under ASan. Compiled by
// tests/test_host_boundary.py.
#define TPX_HOST_TEST 1
#define __HIPRTC__ 1
#define __device__
#define __forceinline__ inline
#define __ffsll(x) __builtin_ffsll(x)
#define __ffs(x) __builtin_ffs(x)
#define __popc(x) __builtin_popcount(x)
#define __popcll(x) __builtin_popcountll(x)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <math.h>
#include <string>
#include <vector>

static inline unsigned long long atomicAdd(unsigned long long* p,
                                           unsigned long long v) {
    unsigned long long o = *p; *p += v; return o;
}
static inline long long __double_as_longlong(double d) {
    long long v; memcpy(&v, &d, 8); return v;
}
static inline double __longlong_as_double(long long v) {
    double d; memcpy(&d, &v, 8); return d;
}

#include "../tuplex_amd/csrc/tpx_rt.hip.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ULL;
static unsigned long long rnd(void) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static double rnd01(void) { return (double)(rnd() >> 11) / 9007199254740992.0; }

typedef std::vector<long long> vll;

// ---- the reference: one byte at a time --------------------------------------

static void serial_stats(const unsigned char* p, long long size, int quotes_on,
                         vll* q, vll* c0, vll* c1) {
    for (long long a = 0; a < size; a += TPX_CSV_CHUNK) {
        long long nq = 0, e = 0, o = 0;
        for (long long i = a; i < size && i < a + TPX_CSV_CHUNK; ++i) {
            if (quotes_on && p[i] == '"') ++nq;
            else if (p[i] == '\n') { if (nq & 1) ++o; else ++e; }
        }
        q->push_back(nq); c0->push_back(e); c1->push_back(o);
    }
}

static void serial_ends(const unsigned char* p, long long size, int quotes_on,
                        vll* ends, vll* per_chunk) {
    bool inside = false;
    per_chunk->assign((size + TPX_CSV_CHUNK - 1) / TPX_CSV_CHUNK, 0);
    for (long long i = 0; i < size; ++i) {
        if (quotes_on && p[i] == '"') inside = !inside;
        else if (p[i] == '\n' && !inside) {
            ends->push_back(i + 1);
            (*per_chunk)[i / TPX_CSV_CHUNK] += 1;
        }
    }
}

// ---- the kernels, lane by lane ----------------------------------------------

// tpx_bs_load_chunk: a whole piece as the 16-byte load, a cut one by the byte
// loop, one past the end not at all
static void host_load(const unsigned char* p, long long cb, long long size,
                      int t, int lane, unsigned w[4]) {
    long long k = cb + t * 1024 + lane * 16;
    if (k + 16 <= size) memcpy(w, p + k, 16);
    else tpx_bs_load_tail((const char*)p, k, size, w);
}

static unsigned lanes_below(unsigned long long m, int lane) {
    return (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}

static void host_chunk_stats(const unsigned char* p, long long size,
                             int quotes_on, vll* q, vll* c0, vll* c1) {
    long long nchunks = (size + TPX_CSV_CHUNK - 1) / TPX_CSV_CHUNK;
    for (long long c = 0; c < nchunks; ++c) {
        unsigned carry = 0, acc[64], accq[64];
        memset(acc, 0, sizeof acc); memset(accq, 0, sizeof accq);
        for (int t = 0; t < 4; ++t) {
            unsigned nq[64], e[64], o[64];
            unsigned long long odd = 0;
            for (int lane = 0; lane < 64; ++lane) {
                unsigned w[4];
                host_load(p, c * TPX_CSV_CHUNK, size, t, lane, w);
                tpx_bs_count16(w[0], w[1], w[2], w[3], quotes_on, &nq[lane],
                               &e[lane], &o[lane]);
                if (nq[lane] & 1u) odd |= 1ull << lane;
            }
            for (int lane = 0; lane < 64; ++lane) {
                unsigned par = (carry ^ lanes_below(odd, lane)) & 1u;
                acc[lane] += par ? (o[lane] | e[lane] << 16)
                                 : (e[lane] | o[lane] << 16);
                accq[lane] += nq[lane];
            }
            carry ^= (unsigned)__popcll(odd);
        }
        unsigned s = 0, sq = 0;
        for (int lane = 0; lane < 64; ++lane) {
            // the packed sum must never carry from the c0 field into c1
            if ((s & 0xFFFFu) + (acc[lane] & 0xFFFFu) > 0xFFFFu) {
                printf("packed field overflow\n"); exit(1);
            }
            s += acc[lane]; sq += accq[lane];
        }
        q->push_back(sq); c0->push_back(s & 0xFFFFu); c1->push_back(s >> 16);
    }
}

static const long long POISON = 0x5A5A5A5A5A5A5A5ALL;

// tpx_csv_emit_rows for rows [row_lo, row_hi]; offs has nrows + 1 entries
static void host_emit_rows(const unsigned char* p, long long size,
                           int quotes_on, const vll& qscan, const vll& base,
                           long long row_lo, long long row_hi, vll* offs) {
    long long nchunks = (long long)base.size();
    long long cap = (long long)offs->size();
    if (row_lo == 0) (*offs)[0] = 0;
    for (long long c = 0; c < nchunks; ++c) {
        if (!(base[c] < row_hi)) continue;
        if (c + 1 < nchunks && base[c + 1] < row_lo) continue;
        unsigned carry = (unsigned)qscan[c] & 1u;
        long long run = base[c];
        for (int t = 0; t < 4; ++t) {
            tpx_bs_det d[64];
            unsigned long long odd = 0;
            for (int lane = 0; lane < 64; ++lane) {
                unsigned w[4];
                host_load(p, c * TPX_CSV_CHUNK, size, t, lane, w);
                tpx_bs_detect(w[0], w[1], w[2], w[3], quotes_on, &d[lane]);
                if (__popc(d[lane].mq) & 1) odd |= 1ull << lane;
            }
            unsigned ex = 0;
            for (int lane = 0; lane < 64; ++lane) {
                unsigned par = (carry ^ lanes_below(odd, lane)) & 1u;
                unsigned r16 = tpx_bs_rows16(&d[lane], par);
                long long idx = run + ex;
                long long k = c * TPX_CSV_CHUNK + t * 1024 + lane * 16;
                ex += (unsigned)__popc(r16);
                while (r16) {
                    if (1 + idx >= cap) { printf("store past row_offs\n"); exit(1); }
                    (*offs)[1 + idx++] = k + __ffs((int)r16);
                    r16 &= r16 - 1;
                }
            }
            carry ^= (unsigned)__popcll(odd) & 1u;
            run += ex;
        }
    }
}

// ---- one input, both kernels -------------------------------------------------

static int g_fails = 0;
static long g_inputs = 0, g_rows = 0;

static void fail(const char* what, long long size, int quotes_on, long long at) {
    if (++g_fails <= 10)
        printf("MISMATCH %s: size %lld quotes_on %d at %lld\n", what, size,
               quotes_on, at);
}

static vll exscan(const vll& v, long long* total) {
    vll out(v.size()); long long s = 0;
    for (size_t i = 0; i < v.size(); ++i) { out[i] = s; s += v[i]; }
    *total = s;
    return out;
}

static void check(const std::string& in, int quotes_on, bool ranged) {
    long long size = (long long)in.size();
    // exact-size block: the byte after the input is not ours to read
    unsigned char* p = (unsigned char*)malloc(size ? size : 1);
    memcpy(p, in.data(), size);
    ++g_inputs;
    vll rq, r0, r1, hq, h0, h1;
    serial_stats(p, size, quotes_on, &rq, &r0, &r1);
    host_chunk_stats(p, size, quotes_on, &hq, &h0, &h1);
    for (size_t c = 0; c < rq.size(); ++c) {
        if (hq[c] != rq[c]) fail("q", size, quotes_on, c);
        if (h0[c] != r0[c]) fail("c0", size, quotes_on, c);
        if (h1[c] != r1[c]) fail("c1", size, quotes_on, c);
    }
    vll ends, rc;
    serial_ends(p, size, quotes_on, &ends, &rc);
    long long tq, nrows;
    vll qscan = exscan(rq, &tq), base = exscan(rc, &nrows);
    g_rows += nrows;
    if (nrows) {
        vll offs(nrows + 1, POISON);
        host_emit_rows(p, size, quotes_on, qscan, base, 0, nrows, &offs);
        if (offs[0] != 0) fail("row_offs[0]", size, quotes_on, 0);
        for (long long r = 0; r < nrows; ++r)
            if (offs[r + 1] != ends[r]) { fail("row_offs", size, quotes_on, r); break; }
        if (ranged) {
            vll edges;
            edges.push_back(0); edges.push_back(nrows);
            for (size_t c = 0; c < base.size(); ++c)
                for (long long dlt = -1; dlt <= 1; ++dlt)
                    if (base[c] + dlt >= 0 && base[c] + dlt <= nrows)
                        edges.push_back(base[c] + dlt);
            for (size_t a = 0; a < edges.size(); ++a)
                for (size_t b = 0; b < edges.size(); ++b) {
                    long long lo = edges[a], hi = edges[b];
                    if (hi <= lo) continue;
                    vll o2(nrows + 1, POISON);
                    host_emit_rows(p, size, quotes_on, qscan, base, lo, hi, &o2);
                    for (long long r = 0; r <= nrows; ++r) {
                        long long want = r ? ends[r - 1] : 0;
                        bool in_range = r >= lo && r <= hi;
                        if (o2[r] != want && (in_range || o2[r] != POISON)) {
                            fail("ranged", size, quotes_on, r);
                            break;
                        }
                    }
                }
        }
    }
    free(p);
}

// '"', '\n', '\r', ',', 'a', the value+1 bytes '#' and 0x0B (what a detect with
// a borrow flags after a true match), and the high-bit twins 0xA2 and 0x8A
static const unsigned char OTHER[] = {'\r', ',', 'a', '#', 0x0B, 0xA2, 0x8A};

static std::string fuzz(long long n, double pq, double pn) {
    std::string s((size_t)n, 'a');
    for (long long i = 0; i < n; ++i) {
        double u = rnd01();
        if (u < pq) s[i] = '"';
        else if (u < pq + pn) s[i] = '\n';
        else s[i] = (char)OTHER[rnd() % sizeof OTHER];
    }
    return s;
}

int main(void) {
    static const long long SIZES[] = {1, 15, 16, 17, 31, 33, 1023, 1024, 1025,
                                      2047, 4095, 4096, 4097, 8191, 8192,
                                      3 * 4096 + 5};
    static const double DENS[] = {0.0, 0.01, 0.1, 0.5, 1.0};
    for (int quotes_on = 0; quotes_on <= 1; ++quotes_on) {
        // the field-width and seam cases
        for (size_t i = 0; i < sizeof SIZES / sizeof *SIZES; ++i) {
            long long n = SIZES[i];
            check(std::string((size_t)n, '\n'), quotes_on, false);
            check(std::string((size_t)n, '"'), quotes_on, false);
            check(std::string((size_t)n, 'a'), quotes_on, false);
            std::string alt((size_t)n, '"'), trap((size_t)n, '\n');
            for (long long j = 0; j < n; ++j) {
                if (j & 1) alt[j] = '\n';
                trap[j] = "\"\n#\n\x0b"[j % 5];
            }
            check(alt, quotes_on, n <= 8191);
            check(trap, quotes_on, false);
            // a quote at each seam byte with a newline on either side
            static const long long SEAM[] = {15, 16, 1023, 1024, 4095, 4096};
            for (size_t k = 0; k < sizeof SEAM / sizeof *SEAM; ++k) {
                long long at = SEAM[k];
                if (at + 1 >= n || at == 0) continue;
                std::string s((size_t)n, 'a');
                s[at - 1] = '\n'; s[at] = '"'; s[at + 1] = '\n';
                s[n - 1] = '\n';
                check(s, quotes_on, false);
            }
        }
        // fuzz: densities from 0 to 1, sizes around every seam
        for (size_t a = 0; a < sizeof DENS / sizeof *DENS; ++a)
            for (size_t b = 0; b < sizeof DENS / sizeof *DENS; ++b) {
                double pq = DENS[a], pn = DENS[b];
                if (pq + pn > 1.0) pn = 1.0 - pq;
                for (int rep = 0; rep < 12; ++rep) {
                    long long n = SIZES[rnd() % (sizeof SIZES / sizeof *SIZES)];
                    if (rep & 1) n = 1 + (long long)(rnd() % 13000);
                    check(fuzz(n, pq, pn), quotes_on, rep < 2 && n <= 8192);
                }
            }
    }
    printf("%ld inputs, %ld rows, %d mismatches\n", g_inputs, g_rows, g_fails);
    if (g_fails) { printf("FAILED\n"); return 1; }
    printf("OK\n");
    return 0;
}
