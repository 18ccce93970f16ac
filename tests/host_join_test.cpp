// Host-compiled driver for the device join table (tuplex_amd/csrc/
// tpx_join.hip.h), used by tests/test_host_join.py: the insert functions run
// sequentially (atomicCAS is a plain compare-and-swap here) and the probe
// functions answer over exact-size heap arrays, so ASan sees any read or
// write past the slot table or a column. Same TPX_HOST_TEST macro set as
// host_re_test.cpp.
//
// stdin:   I <n> <k0> <k1> ...          build an i64-key table
//          S <n> <hex|-> ...            build a str-key table
//          p <key>                      probe the i64 table
//          q <hex|->                    probe the str table
// stdout:  per build  "B <tsize> <occupied> <lost>"
//          per probe  "<row>"   (lost = inserts that found no slot)
#define TPX_HOST_TEST 1
#define __HIPRTC__ 1
#define __device__
#define __forceinline__ inline
#define __ffsll(x) __builtin_ffsll(x)
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
static inline int atomicCAS(int* p, int cmp, int v) {
    int o = *p; if (o == cmp) *p = v; return o;
}
static inline unsigned long long atomicCAS(unsigned long long* p,
                                           unsigned long long cmp,
                                           unsigned long long v) {
    unsigned long long o = *p; if (o == cmp) *p = v; return o;
}
static inline long long __double_as_longlong(double d) {
    long long v; memcpy(&v, &d, 8); return v;
}
static inline double __longlong_as_double(long long v) {
    double d; memcpy(&d, &v, 8); return d;
}

#include "../tuplex_amd/csrc/tpx_rt.hip.h"

// the two hashes live in the device-only part of tpx_rt.hip.h; these are
// the same functions (the python side checks them against
// codegen._jhash_i64 / _jhash_bytes through the slots they pick)
static inline unsigned long long tpx_jhash_bytes(const char* p, long long n) {
    unsigned long long h = 1469598103934665603ULL;
    for (long long i = 0; i < n; ++i) {
        h ^= (unsigned char)p[i];
        h *= 1099511628211ULL;
    }
    return h;
}
static inline unsigned long long tpx_hash_i64(long long k) {
    unsigned long long x = (unsigned long long)k;
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}

#include "../tuplex_amd/csrc/tpx_join.hip.h"

static int hexv(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

static std::string unhex(const char* s) {
    std::string out;
    if (s[0] == '-') return out;
    for (size_t i = 0; hexv(s[i]) >= 0 && hexv(s[i + 1]) >= 0; i += 2)
        out.push_back((char)(hexv(s[i]) * 16 + hexv(s[i + 1])));
    return out;
}

struct Table {
    TpxJoinTab t;
    void* slots = nullptr;
    long long* keys = nullptr;   // i64 key column / str offsets
    char* bytes = nullptr;
    void release() {
        free(slots); free(keys); free(bytes);
        slots = nullptr; keys = nullptr; bytes = nullptr;
    }
};

static unsigned long long table_size(long long n) {
    unsigned long long tsize = 8;
    while (tsize < 2ULL * (unsigned long long)(n > 0 ? n : 1)) tsize <<= 1;
    return tsize;
}

int main(void) {
    Table ti, ts;
    memset(&ti.t, 0, sizeof ti.t);
    memset(&ts.t, 0, sizeof ts.t);
    bool have_i = false, have_s = false;
    std::string line;
    int ch;
    for (;;) {
        line.clear();
        while ((ch = getchar()) != EOF && ch != '\n') line.push_back((char)ch);
        if (line.empty() && ch == EOF) break;
        if (line.empty()) continue;
        char* q = &line[1];
        if (line[0] == 'I') {
            ti.release();
            long long n = strtoll(q, &q, 10);
            unsigned long long tsize = table_size(n);
            ti.keys = (long long*)malloc((size_t)(n ? n : 1) * 8);
            for (long long i = 0; i < n; ++i) ti.keys[i] = strtoll(q, &q, 10);
            TpxJoinSlotI* sl =
                (TpxJoinSlotI*)malloc((size_t)tsize * sizeof(TpxJoinSlotI));
            memset(sl, 0xFF, (size_t)tsize * sizeof(TpxJoinSlotI));
            ti.slots = sl;
            long long lost = 0;
            for (long long i = 0; i < n; ++i)
                if (tpx_join_insert_i64(sl, tsize - 1, ti.keys[i], (int)i) < 0)
                    ++lost;
            memset(&ti.t, 0, sizeof ti.t);
            ti.t.slots = sl;
            ti.t.mask = tsize - 1;
            ti.t.n_rows = n;
            ti.t.n_cols = 1;
            ti.t.key_col = 0;
            ti.t.cols[0] = ti.keys;
            long long occ = 0;
            for (unsigned long long s = 0; s < tsize; ++s)
                if (sl[s].row >= 0) ++occ;
            printf("B %llu %lld %lld\n", tsize, occ, lost);
            have_i = true;
        } else if (line[0] == 'S') {
            ts.release();
            long long n = strtoll(q, &q, 10);
            unsigned long long tsize = table_size(n);
            std::vector<std::string> keys;
            for (long long i = 0; i < n; ++i) {
                while (*q == ' ') ++q;
                keys.push_back(unhex(q));
                while (*q && *q != ' ') ++q;
            }
            ts.keys = (long long*)malloc((size_t)(n + 1) * 8);
            size_t total = 0;
            for (long long i = 0; i < n; ++i) {
                ts.keys[i] = (long long)total;
                total += keys[(size_t)i].size();
            }
            ts.keys[n] = (long long)total;
            ts.bytes = (char*)malloc(total ? total : 1);
            for (long long i = 0; i < n; ++i)
                if (!keys[(size_t)i].empty())
                    memcpy(ts.bytes + ts.keys[i], keys[(size_t)i].data(),
                           keys[(size_t)i].size());
            unsigned long long* sl =
                (unsigned long long*)malloc((size_t)tsize * 8);
            memset(sl, 0xFF, (size_t)tsize * 8);
            ts.slots = sl;
            long long lost = 0;
            for (long long i = 0; i < n; ++i)
                if (tpx_join_insert_str(sl, tsize - 1, ts.bytes + ts.keys[i],
                                        ts.keys[i + 1] - ts.keys[i],
                                        (int)i) < 0)
                    ++lost;
            memset(&ts.t, 0, sizeof ts.t);
            ts.t.slots = sl;
            ts.t.mask = tsize - 1;
            ts.t.n_rows = n;
            ts.t.n_cols = 1;
            ts.t.key_col = 0;
            ts.t.cols[0] = ts.keys;
            ts.t.cols[1] = ts.bytes;
            long long occ = 0;
            for (unsigned long long s = 0; s < tsize; ++s)
                if (sl[s] != TPX_JOIN_EMPTY64) ++occ;
            printf("B %llu %lld %lld\n", tsize, occ, lost);
            have_s = true;
        } else if (line[0] == 'p') {
            if (!have_i) { fprintf(stderr, "p before I\n"); return 2; }
            printf("%d\n", tpx_join_probe_i64(ti.t, strtoll(q, &q, 10)));
        } else if (line[0] == 'q') {
            if (!have_s) { fprintf(stderr, "q before S\n"); return 2; }
            while (*q == ' ') ++q;
            std::string k = unhex(q);
            // exact-size heap copy: ASan sees any read past the key
            char* kp = (char*)malloc(k.size() ? k.size() : 1);
            if (!k.empty()) memcpy(kp, k.data(), k.size());
            printf("%d\n", tpx_join_probe_str(ts.t, tstr{kp, (long long)k.size()}));
            free(kp);
        } else {
            fprintf(stderr, "bad line\n");
            return 2;
        }
    }
    ti.release();
    ts.release();
    printf("OK\n");
    return 0;
}
