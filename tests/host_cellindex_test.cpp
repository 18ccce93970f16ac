// Host-compiled check of the wave-cooperative cell index (csrc/tpx_ci.hip.h):
// the 64 lanes are emulated one after another with a plain-C stand-in for the
// ballot / exscan glue of tpx_ci_stage that calls the same per-lane functions
// (tpx_ci_classify, tpx_ci_inq, tpx_ci_scatter), and every row is then read
// back through tpx_ci_row / tpx_ci_cell and compared with tpx_csv_next_cell.
// A row may decline; an accepted row must equal the reference exactly (p, n,
// flags, avail protocol, ASCII gate). A declined row goes through
// tpx_mw_cell, as in the kernel. Compiled by tests/test_host_cellindex.py.
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
#include "../tuplex_amd/csrc/tpx_ci.hip.h"

static unsigned long long rng_state = 88172645463325252ULL;
static unsigned long long rnd(void) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

#define SPAN_CAP 16344
#define CANARY 64
static const unsigned char CANARY_BYTE = 0xA5;

// LDS stand-ins: the staged span (+80 B tail the walk may overread) and the
// index region with a canary behind it
alignas(16) static char g_lds[SPAN_CAP + 80 + 64];
alignas(16) static unsigned char g_ci[TPX_CI_BYTES + CANARY];

// tpx_ci_stage with the wave glue in plain C. `src` = span bytes, lo = first
// row's start in the span. Returns the uniform "index usable" flag.
static bool host_ci_stage(const char* src, int span, int lo, char delim) {
    char* ci = (char*)g_ci;
    unsigned* ent = (unsigned*)(ci + TPX_CI_ENT_OFF);
    unsigned short* rf = (unsigned short*)(ci + TPX_CI_RF_OFF);
    unsigned long long* bad = (unsigned long long*)(ci + TPX_CI_BAD_OFF);
    for (int lane = 0; lane < 64; ++lane) rf[lane + 1] = (unsigned short)TPX_CI_NONE;
    rf[0] = 0;
    unsigned car_ord = 0, car_nl = 0, car_q = 0;
    bool pend = false;
    int trip = 0;
    for (int kb = 0; kb < span; kb += 64 * 16, ++trip) {
        tpx_ci_cls c[64];
        unsigned pq[64], s16[64], n16[64], ps[64], pn[64];
        unsigned long long oddm = 0;
        for (int lane = 0; lane < 64; ++lane) {
            int k = kb + lane * 16;
            unsigned w[4] = {0, 0, 0, 0};
            for (int j = k; j < span && j < k + 16; ++j) {
                unsigned char ch = (unsigned char)src[j];
                g_lds[j] = (char)ch;
                w[(j - k) >> 2] |= (unsigned)ch << (8 * ((j - k) & 3));
            }
            int nv = span - k; nv = nv < 0 ? 0 : (nv > 16 ? 16 : nv);
            int nl_ = lo - k; nl_ = nl_ < 0 ? 0 : (nl_ > 16 ? 16 : nl_);
            unsigned valid = ((1u << nv) - 1u) & ~((1u << nl_) - 1u);
            tpx_ci_classify(w[0], w[1], w[2], w[3], delim, valid, &c[lane]);
            pq[lane] = (unsigned)__popc(c[lane].q);
            if (pq[lane] & 1u) oddm |= 1ull << lane;
        }
        unsigned long long nlf = 0;
        for (int lane = 0; lane < 64; ++lane) {
            unsigned long long below = (1ull << lane) - 1ull;
            unsigned par = (car_q ^ (unsigned)__popcll(oddm & below)) & 1u;
            unsigned inq = tpx_ci_inq(c[lane].q, par);
            s16[lane] = c[lane].s & ~inq;
            n16[lane] = c[lane].n & ~inq;
            ps[lane] = (unsigned)__popc(s16[lane]);
            pn[lane] = (unsigned)__popc(n16[lane]);
            if (n16[lane] & 1u) nlf |= 1ull << lane;
        }
        unsigned long long bw = 0;
        bool newpend = false;
        unsigned xs = 0, xn = 0, xq = 0;  // exclusive prefixes
        for (int lane = 0; lane < 64; ++lane) {
            // the packed 11/11/10-bit fields must hold every exclusive prefix
            if (xs > 0x7FFu || xn > 0x7FFu || xq > 0x3FFu) {
                printf("packed scan field overflow\n"); exit(1);
            }
            unsigned nxt = lane < 63 ? (unsigned)((nlf >> (lane + 1)) & 1ull) : 0u;
            unsigned badr = c[lane].r & ~((n16[lane] >> 1) | (nxt << 15));
            if (lane == 63) { newpend = (badr & 0x8000u) != 0; badr &= 0x7FFFu; }
            if (c[lane].h != 0 || badr != 0) bw |= 1ull << lane;
            tpx_ci_scatter(ci, kb + lane * 16, s16[lane], n16[lane], c[lane].q,
                           car_ord + xs, car_nl + xn, car_q + xq);
            xs += ps[lane]; xn += pn[lane]; xq += pq[lane];
        }
        if (pend && !(nlf & 1ull)) bad[trip - 1] |= 1ull << 63;
        bad[trip] = bw;
        pend = newpend;
        car_ord += xs; car_nl += xn; car_q += xq;
    }
    if (pend) bad[trip - 1] |= 1ull << 63;
    bool ok = car_ord < TPX_CI_CAP;
    if (ok && car_nl < 64) {
        ent[car_ord] = (unsigned)span | (car_q << 16);
        rf[car_nl + 1] = (unsigned short)(car_ord + 1);
    }
    return ok;
}

static int g_fails = 0;
static long g_accepted = 0, g_declined = 0;

struct Batch {
    std::string bytes;            // `pad` bytes of the previous row, then rows
    std::vector<int> offs;        // row offsets into bytes (size rows+1)
    std::vector<int> must_accept; // per row: 1 = the contract says accept
};

static void reset_region(void) {
    memset(g_ci, 0xEE, TPX_CI_BYTES);
    memset(g_ci + TPX_CI_BYTES, CANARY_BYTE, CANARY);
    memset(g_lds, 0, sizeof g_lds);
}

static bool canary_ok(void) {
    for (int i = 0; i < CANARY; ++i)
        if (g_ci[TPX_CI_BYTES + i] != CANARY_BYTE) return false;
    return true;
}

// build the index of a batch (rows start at pad, span start = 0 as the kernel
// rounds it down to 16) and compare every row with the reference walk.
// -> the uniform usable flag
static bool check_batch(const Batch& B, int ncols, const char* what) {
    int span = (int)B.bytes.size();
    int rows = (int)B.offs.size() - 1;
    if (span > SPAN_CAP || rows < 1 || rows > 64) { printf("bad batch\n"); exit(1); }
    reset_region();
    bool ok = host_ci_stage(B.bytes.data(), span, B.offs[0], ',');
    if (!canary_ok()) {
        printf("%s: write past the index region\n", what); ++g_fails; return ok;
    }
    for (int r = 0; r < rows; ++r) {
        int rs = B.offs[r], re = B.offs[r + 1];
        const char* rp = g_lds + rs;
        const char* rend = g_lds + re;
        if (rend > rp && rend[-1] == '\n') --rend;
        if (rend > rp && rend[-1] == '\r') --rend;
        // reference
        tpx_cell ref[32]; bool ref_avail[32]; unsigned long long hib = 0;
        bool avail = true, m = true;
        const char* cur = rp;
        for (int k = 0; k < ncols; ++k) {
            ref_avail[k] = avail;
            if (!avail) { ref[k] = tpx_cell{rp, 0, 0}; continue; }
            cur = tpx_csv_next_cell(cur, rend, &ref[k], &m, ',', &hib);
            avail = m;
        }
        bool ref_over = avail;
        int e0 = 0;
        int fast = ok && tpx_ci_row(g_lds, (const char*)g_ci, r, rs, re,
                                    (int)(rend - g_lds), span, ncols, &e0);
        if (!fast) {
            ++g_declined;
            if (B.must_accept[r] && ok) {
                printf("%s: row %d declined but must be accepted [%.*s]\n",
                       what, r, re - rs, g_lds + rs);
                ++g_fails;
            }
            // declined: the unchanged mask walk
            tpx_mwalk S; tpx_mw_init(S, rp, rend);
            bool av = true;
            for (int k = 0; k < ncols; ++k) {
                if (av != ref_avail[k]) { printf("%s: walk avail\n", what); ++g_fails; break; }
                if (!av) continue;
                tpx_cell c; tpx_mw_cell(S, &c, ',', 0);
                av = S.more;
                if (c.p != ref[k].p || c.n != ref[k].n || c.flags != ref[k].flags) {
                    printf("%s: walk cell\n", what); ++g_fails; break;
                }
            }
            continue;
        }
        ++g_accepted;
        // accepted: every cell available, none left over, no bad flag, ASCII
        bool good = !ref_over && hib == 0;
        for (int k = 0; k < ncols && good; ++k) {
            tpx_cell c{rp, 0, 0};
            tpx_ci_cell(g_lds, (const char*)g_ci, e0, k, ncols, rs,
                        (int)(rend - g_lds), &c);
            good = ref_avail[k] && c.p == ref[k].p && c.n == ref[k].n &&
                   c.flags == ref[k].flags && !(c.flags & 6);
        }
        if (!good) {
            printf("%s: accepted row %d differs from the reference [%.*s]\n",
                   what, r, re - rs, g_lds + rs);
            ++g_fails;
        }
        if (g_fails > 8) return ok;
    }
    return ok;
}

// pad bytes that belong to "the previous row": anything, ending in '\n'
static void add_pad(Batch& B, int pad) {
    const char* junk = "x\",\r\xc3y";
    for (int i = 0; i < pad; ++i)
        B.bytes.push_back(i == pad - 1 ? '\n' : junk[rnd() % 7]);
}

// (a) adversarial fuzz: random bytes; a row ends at every even-parity '\n'
static void fuzz_batch(void) {
    const char* alpha = "ab,\"\r\n x9\xc3\x00-#\x0e|}";
    int alpha_n = 16;
    Batch B;
    int pad = (int)(rnd() % 16);
    add_pad(B, pad);
    int rows = 1 + (int)(rnd() % 64);
    int ncols = 1 + (int)(rnd() % 12);
    bool open_end = (rnd() % 8) == 0;   // last row without a newline
    int style = (int)(rnd() % 3);       // 0 wild, 1 mostly structured, 2 mix
    B.offs.push_back(pad);
    for (int r = 0; r < rows; ++r) {
        int par = 0;
        int maxlen = 5 + (int)(rnd() % 200);
        bool last_open = open_end && r == rows - 1;
        for (int i = 0;; ++i) {
            char c;
            if (style == 0 || (style == 2 && (rnd() & 1)))
                c = (rnd() % 100) < 80 ? alpha[rnd() % alpha_n]
                                       : (char)('a' + rnd() % 26);
            else {
                unsigned t = (unsigned)(rnd() % 100);
                c = t < 12 ? ',' : t < 16 ? '"' : t < 18 ? '\n' :
                    t < 19 ? '\r' : t < 20 ? '\xc3' : (char)('a' + rnd() % 26);
            }
            if (i >= maxlen) {           // close the row
                if (par) { B.bytes.push_back('"'); par = 0; }
                if (last_open) break;
                if ((rnd() & 3) == 0) B.bytes.push_back('\r');
                B.bytes.push_back('\n');
                break;
            }
            if (c == '\n' && !par) {
                if (last_open) c = 'n'; else { B.bytes.push_back(c); break; }
            }
            if (c == '"') par ^= 1;
            B.bytes.push_back(c);
        }
        if ((int)B.bytes.size() == B.offs.back()) B.bytes.push_back('z');  // no empty last row
        B.offs.push_back((int)B.bytes.size());
        B.must_accept.push_back(0);
    }
    if ((int)B.bytes.size() > SPAN_CAP) return;
    check_batch(B, ncols, "fuzz");
}

// (b) structured rows
enum { K_PLAIN, K_EMPTY, K_QCOMMA, K_QNL, K_QEMPTY, K_CLEAN_KINDS,
       // odd kinds: rows holding one of these must decline or match
       K_ESC = K_CLEAN_KINDS, K_STRAY, K_JUNK, K_BARECR, K_UTF8, K_ALL_KINDS };

static std::string make_cell(int kind) {
    std::string s;
    int n = 1 + (int)(rnd() % 9);
    switch (kind) {
    case K_PLAIN: for (int i = 0; i < n; ++i) s.push_back("ab x9-#.}"[rnd() % 9]); break;
    case K_EMPTY: break;
    case K_QCOMMA: s = "\"a,b"; for (int i = 0; i < n; ++i) s.push_back(i & 1 ? ',' : 'q'); s += "\""; break;
    case K_QNL: s = "\"l1\nl2"; if (rnd() & 1) s += "\n,x"; s += "\""; break;
    case K_QEMPTY: s = "\"\""; break;
    case K_ESC: s = "\"he said \"\"hi\"\"\""; break;
    case K_STRAY: s = "ab\"cd\"e"; break;       // even count keeps the row one row
    case K_JUNK: s = "\"q\"junk"; break;
    case K_BARECR: s = "a\rb"; break;
    case K_UTF8: s = "n\xc3\xa9"; break;
    }
    return s;
}

static void structured_batch(int ncols, bool crlf, bool open_end, bool odd,
                             int rows) {
    Batch B;
    int pad = (int)(rnd() % 16);
    add_pad(B, pad);
    B.offs.push_back(pad);
    for (int r = 0; r < rows; ++r) {
        bool clean = true;
        int nc = ncols;
        if (odd && (rnd() % 4) == 0) {           // wrong cell count
            nc = (rnd() & 1) ? ncols + 1 : ncols - 1;
            clean = false;
        }
        for (int k = 0; k < nc; ++k) {
            int kind = (int)(rnd() % K_CLEAN_KINDS);
            if (odd && (rnd() % 6) == 0) {
                kind = K_CLEAN_KINDS + (int)(rnd() % (K_ALL_KINDS - K_CLEAN_KINDS));
                clean = false;
            }
            if (k) B.bytes.push_back(',');
            B.bytes += make_cell(kind);
        }
        bool last_open = open_end && r == rows - 1;
        if (!last_open) { if (crlf) B.bytes.push_back('\r'); B.bytes.push_back('\n'); }
        if ((int)B.bytes.size() == B.offs.back()) {  // an empty open last row
            B.bytes.push_back('z'); clean = clean && ncols == 1;
        }
        B.offs.push_back((int)B.bytes.size());
        B.must_accept.push_back(clean ? 1 : 0);
    }
    // a neighbour's high byte / CR may share a 16-B block with a clean row:
    // only rows of batches without odd rows MUST be accepted
    if (odd) for (size_t i = 0; i < B.must_accept.size(); ++i) B.must_accept[i] = 0;
    // the pad belongs to the previous row and is masked out, whatever it holds
    if ((int)B.bytes.size() > SPAN_CAP) return;
    check_batch(B, ncols, odd ? "structured+odd" : "structured");
}

// (c) more structural bytes than the list holds
static void overflow_batch(void) {
    Batch B;
    B.offs.push_back(0);
    for (int r = 0; r < 64; ++r) {
        for (int k = 0; k < 20; ++k) B.bytes += "a,";
        B.bytes += "z\n";
        B.offs.push_back((int)B.bytes.size());
        B.must_accept.push_back(0);
    }
    bool ok = check_batch(B, 21, "overflow");     // 64*21 entries > capacity
    if (ok) { printf("overflow: batch flag not raised\n"); ++g_fails; }
    // all commas, one row: far above the capacity in a single trip
    Batch C;
    C.offs.push_back(0);
    C.bytes.assign(4000, ',');
    C.bytes.push_back('\n');
    C.offs.push_back((int)C.bytes.size());
    C.must_accept.push_back(0);
    ok = check_batch(C, 12, "overflow2");
    if (ok) { printf("overflow2: batch flag not raised\n"); ++g_fails; }
    // exactly at the limit: 64 rows x 14 columns fits
    Batch D;
    D.offs.push_back(0);
    for (int r = 0; r < 64; ++r) {
        for (int k = 0; k < 13; ++k) D.bytes += "a,";
        D.bytes += "z\n";
        D.offs.push_back((int)D.bytes.size());
        D.must_accept.push_back(1);
    }
    ok = check_batch(D, 14, "limit");
    if (!ok) { printf("limit: 64 x 14 must fit\n"); ++g_fails; }
}

int main(void) {
    static_assert(64 * 14 + 1 <= TPX_CI_CAP, "14 columns fit");
    static_assert(TPX_CI_ENT_OFF + 4 * TPX_CI_CAP <= TPX_CI_BYTES, "layout");
    static_assert(TPX_CI_RF_OFF + 2 * 65 <= TPX_CI_BAD_OFF, "layout");
    static_assert(TPX_CI_BAD_OFF + 8 * 16 <= TPX_CI_ENT_OFF, "layout");
    // every span-start misalignment 0..15 with 1..64 rows is drawn many
    // times over (pad and rows are uniform)
    for (int it = 0; it < 6000 && g_fails <= 8; ++it) fuzz_batch();
    long fz_acc = g_accepted, fz_dec = g_declined;
    for (int it = 0; it < 4000 && g_fails <= 8; ++it) {
        int ncols = 1 + (int)(rnd() % 14);
        int rows = 1 + (int)(rnd() % 64);
        structured_batch(ncols, (it & 1) != 0, (it & 6) == 2, false, rows);
    }
    long st_dec = g_declined - fz_dec;
    if (st_dec != 0) {
        printf("structured: %ld clean rows declined (cap 0)\n", st_dec);
        ++g_fails;
    }
    for (int it = 0; it < 4000 && g_fails <= 8; ++it) {
        int ncols = 1 + (int)(rnd() % 14);
        int rows = 1 + (int)(rnd() % 64);
        structured_batch(ncols, (it & 1) != 0, (it & 6) == 2, true, rows);
    }
    overflow_batch();
    printf("fuzz accepted %ld declined %ld; total accepted %ld declined %ld\n",
           fz_acc, fz_dec, g_accepted, g_declined);
    if (fz_acc < 1000) { printf("fuzz accepts too few rows to mean much\n"); ++g_fails; }
    if (g_fails) { printf("FAIL %d\n", g_fails); return 1; }
    printf("OK\n");
    return 0;
}
