// Host-compiled check of the per-lane pieces of the cache() pack
// (csrc/tpx_cache.hip.h): tpx_cp_len, tpx_cp_move for every descriptor kind,
// and tpx_cp_owner — the six-step search a lane of tpx_cache_gather_str uses
// to find the row that owns its destination byte. The 64 lanes of a batch are
// emulated one after another with a plain-C stand-in for the wave glue (the
// prefix arrays take the place of the lane shuffles), and the destination is
// compared with a row-by-row memcpy, canaries on both sides. Compiled by
// tests/test_host_cachepack.py, plain and under ASan+UBSan.
#define TPX_HOST_TEST 1
#define __device__
#define __forceinline__ inline
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <vector>

#include "../tuplex_amd/csrc/tpx_cache.hip.h"

static unsigned long long rng_state = 88172645463325252ULL;
static unsigned long long rnd(void) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);           \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

static const int LENS[] = {0, 1, 7, 8, 9, 63, 64, 65, 700};

// one 64-row batch of tpx_cache_gather_str, lanes in sequence
static void host_gather_batch(const unsigned char* keep, const int* slen,
                              const unsigned char* snull, const char** sptr,
                              int nrows, char* dst, long long* total_out) {
    long long len[64], before[64];
    unsigned incl[64], excl[64];
    long long run = 0;
    for (int l = 0; l < 64; ++l) {
        bool kept = l < nrows && keep[l];
        len[l] = kept ? tpx_cp_len(slen[l], snull && snull[l]) : 0;
        before[l] = run;
        run += len[l];
        incl[l] = (unsigned)(before[l] + len[l]);
        excl[l] = (unsigned)before[l];
    }
    long long total = run;
    *total_out = total;
    for (long long base = 0; base < total; base += 64) {
        for (int lane = 0; lane < 64; ++lane) {
            long long j = base + lane;
            bool live = j < total;
            unsigned jj = (unsigned)(live ? j : total - 1);
            int o = tpx_cp_owner([&](int k) { return incl[k]; }, jj);
            CHECK(o >= 0 && o < 64 && len[o] > 0);
            CHECK(excl[o] <= jj && jj < incl[o]);
            if (live) dst[j] = sptr[o][jj - excl[o]];
        }
    }
}

static void test_gather(int rounds) {
    for (int round = 0; round < rounds; ++round) {
        static const int first[8] = {1, 2, 63, 64, 64, 64, 17, 33};
        int nrows = round < 8 ? first[round] : 1 + (int)(rnd() % 64);
        std::vector<std::vector<char>> cells(64);
        unsigned char keep[64], snull[64];
        int slen[64];
        const char* sptr[64];
        int pattern = round % 6;
        for (int l = 0; l < 64; ++l) {
            int L = LENS[rnd() % 9];
            if (round % 11 == 3) L = (int)(rnd() % 3);  // mostly empty cells
            cells[l].resize((size_t)L + 8);
            for (auto& ch : cells[l]) ch = (char)(rnd() & 0xFF);
            sptr[l] = cells[l].data() + (l & 7);  // every alignment
            slen[l] = L > (l & 7) ? L - (l & 7) : 0;
            snull[l] = (rnd() % 5) == 0;
            keep[l] = pattern == 0 ? 1 : pattern == 1 ? 0
                    : pattern == 2 ? (l & 1) : pattern == 3 ? (l == 0)
                    : pattern == 4 ? (l == nrows - 1) : (rnd() & 1);
            if (snull[l] && (l & 3) == 0) slen[l] = -5;  // garbage under null
        }
        // reference: row by row
        std::vector<char> want;
        for (int l = 0; l < nrows; ++l) {
            if (!keep[l] || snull[l] || slen[l] <= 0) continue;
            want.insert(want.end(), sptr[l], sptr[l] + slen[l]);
        }
        std::vector<char> dst(want.size() + 128, (char)0xA5);
        long long total = -1;
        host_gather_batch(keep, slen, snull, sptr, nrows, dst.data() + 64,
                          &total);
        CHECK(total == (long long)want.size());
        CHECK(want.empty() ||
              memcmp(dst.data() + 64, want.data(), want.size()) == 0);
        for (int b = 0; b < 64; ++b) {
            CHECK(dst[(size_t)b] == (char)0xA5);
            CHECK(dst[64 + want.size() + (size_t)b] == (char)0xA5);
        }
    }
}

static void test_owner_exhaustive_small(void) {
    // every destination byte of random length vectors against a linear walk
    for (int round = 0; round < 2000; ++round) {
        unsigned incl[64];
        unsigned run = 0;
        for (int l = 0; l < 64; ++l) {
            unsigned L = (rnd() % 4 == 0) ? 0 : (unsigned)(rnd() % 40);
            if (l == 63 && run == 0) L = 1;
            run += L;
            incl[l] = run;
        }
        for (unsigned j = 0; j < run; ++j) {
            int want = 0;
            while (incl[want] <= j) ++want;
            CHECK(tpx_cp_owner([&](int k) { return incl[k]; }, j) == want);
        }
    }
}

static void test_move(void) {
    const int n = 9;
    long long val8[n], bools[n];
    unsigned char mask[n];
    int lens[n];
    for (int i = 0; i < n; ++i) {
        val8[i] = (long long)rnd();
        bools[i] = (i % 3 == 0) ? 0 : (i % 3 == 1 ? 1 : (long long)rnd() | 2);
        mask[i] = (unsigned char)((i & 1) ? 0x80 : 0);
        lens[i] = i == 4 ? -1 : i * 100;
    }
    long long o8[n + 1];
    unsigned char ob[n + 1], om[n + 1];
    long long ol[n + 1];
    memset(o8, 0xA5, sizeof o8); memset(ob, 0xA5, sizeof ob);
    memset(om, 0xA5, sizeof om); memset(ol, 0xA5, sizeof ol);
    tpx_cp_desc d8{val8, o8, nullptr, TPX_CP_VAL8};
    tpx_cp_desc db{bools, ob, nullptr, TPX_CP_BOOL};
    tpx_cp_desc dm{mask, om, nullptr, TPX_CP_MASK};
    tpx_cp_desc dl{lens, ol, mask, TPX_CP_LEN};
    for (int i = 0; i < n; ++i) {
        int r = n - 1 - i;  // any rank
        tpx_cp_move(d8, i, r); tpx_cp_move(db, i, r);
        tpx_cp_move(dm, i, r); tpx_cp_move(dl, i, r);
    }
    for (int i = 0; i < n; ++i) {
        int r = n - 1 - i;
        CHECK(o8[r] == val8[i]);
        CHECK(ob[r] == (bools[i] != 0 ? 1 : 0));
        CHECK(om[r] == (mask[i] ? 1 : 0));
        CHECK(ol[r] == ((mask[i] || lens[i] < 0) ? 0 : lens[i]));
    }
    CHECK(ob[n] == 0xA5 && om[n] == 0xA5);
    CHECK(tpx_cp_len(7, false) == 7 && tpx_cp_len(7, true) == 0 &&
          tpx_cp_len(-7, false) == 0 && tpx_cp_len(0, false) == 0);
    CHECK(sizeof(tpx_cp_desc) == 32);
}

int main(void) {
    test_move();
    test_owner_exhaustive_small();
    test_gather(600);
    printf("OK\n");
    return 0;
}
