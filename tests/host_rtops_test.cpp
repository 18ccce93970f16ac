// Host-compiled differential driver for the scalar device runtime
// (tuplex_amd/csrc/tpx_rt.hip.h): every helper a generated kernel calls is run
// here on cases that tests/test_host_rtops.py generates and checks against
// CPython / the oracle. Built twice by that test (plain -O2, and ASan+UBSan);
// a stand-alone executable, nothing is loaded into Python.
//
// stdin, one case per line:   <op> <shift> <pad> <cap> <args...>
//   shift  0..7   alignment of every subject string
//   pad    0..255 byte the subject arena is filled with (the needle byte, so
//                 an over-read that influences a result gives a wrong answer)
//   cap    heap capacity in bytes for this case (<= HEAP_MAX)
//   args   per-op (table below): s = hex bytes ("-" = empty), i = integer,
//          d = double as 16 hex digits
// stdout, one line per case: "E<ec>" when the op set an error code, else the
// result (strings hex, doubles as bit patterns, the rest integers). A violated
// memory contract prints "MEMFAIL <why>" instead. Ends with per-op counts on
// stderr and "OK" on stdout.
//
// Memory layout mirrors the device contract and nothing more generous: each
// subject string k sits at arena + 64 + shift + 8*m (all at alignment `shift`)
// with >= 16 pad bytes before, between and after; the arena is malloc'd to
// exactly that size so ASan sees anything beyond. Outputs go through a real
// TpxHeap over a canary-filled host buffer with guard zones; after each case
// the arena must be unchanged and the heap untouched outside [0, cursor)
// (outside the result inside it; entirely, when an error code was set).
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
#include <map>
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

#define HEAP_MAX 8192
#define GUARD 64
#define CANARY ((char)0xA5)

static const char* const SIGS[][2] = {
    {"memchr", "si"}, {"memchr_hi", "si"}, {"memchr2", "sii"},
    {"memrchr", "si"}, {"memchr_hi_spec", "sii"}, {"ascii", "s"},
    {"csv_needs_quote", "s"}, {"csv_cell_len", "s"}, {"csv_cell_write", "s"},
    {"memcpy", "si"},
    {"find", "ss"}, {"rfind", "ss"}, {"contains", "ss"}, {"startswith", "ss"},
    {"endswith", "ss"}, {"streq", "ss"}, {"strcmp", "ss"}, {"getitem", "si"},
    {"slice", "siiii"}, {"center", "sis"}, {"strmul", "si"}, {"lower", "s"},
    {"upper", "s"}, {"swapcase", "s"}, {"capitalize_ix", "s"}, {"strip", "s"},
    {"concat", "ss"}, {"replace", "sss"}, {"splitget", "ssi"},
    {"int_drop", "ss"},
    {"atoi", "s"}, {"atod", "s"}, {"int_str", "s"}, {"float_str", "s"},
    {"cell_i64", "s"}, {"cell_f64", "s"}, {"cell_bool", "s"},
    {"floordiv_i64", "ii"}, {"mod_i64", "ii"}, {"truediv", "dd"},
    {"floordiv_f64", "dd"}, {"mod_f64", "dd"}, {"int_f64", "d"},
    {"i64_digits", "i"}, {"i64_write", "i"}, {"str_i64", "i"},
    {"fmt0d", "ii"}, {"f64_csv", "d"}, {"csv_row", "si"},
};

static int hexval(char c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

static std::string unhex(const std::string& t) {
    std::string o;
    if (t == "-") return o;
    for (size_t i = 0; i + 1 < t.size(); i += 2)
        o.push_back((char)(hexval(t[i]) * 16 + hexval(t[i + 1])));
    return o;
}

static void put_hex(std::string& o, const char* p, long long n) {
    static const char* d = "0123456789abcdef";
    if (n < 0) { o += "NEGLEN"; return; }
    if (n == 0) { o += "-"; return; }
    for (long long i = 0; i < n; ++i) {
        o.push_back(d[((unsigned char)p[i]) >> 4]);
        o.push_back(d[((unsigned char)p[i]) & 15]);
    }
}

static void put_i(std::string& o, long long v) {
    char b[32]; snprintf(b, sizeof b, "%lld", v); o += b;
}

static void put_d(std::string& o, double v) {
    char b[32];
    snprintf(b, sizeof b, "%016llx", (unsigned long long)__double_as_longlong(v));
    o += b;
}

static double get_d(const std::string& t) {
    return __longlong_as_double((long long)strtoull(t.c_str(), nullptr, 16));
}

int main(void) {
    std::map<std::string, std::string> sigs;
    std::map<std::string, long long> counts;
    for (auto& s : SIGS) sigs[s[0]] = s[1];

    char* heapbuf = (char*)malloc(GUARD + HEAP_MAX + GUARD);
    char* canary = (char*)malloc(GUARD + HEAP_MAX + GUARD);
    memset(canary, CANARY, GUARD + HEAP_MAX + GUARD);
    memset(heapbuf, CANARY, GUARD + HEAP_MAX + GUARD);
    char* hb = heapbuf + GUARD;

    char* line = nullptr;
    size_t lcap = 0;
    long long lineno = 0;
    std::vector<std::string> tok;
    std::string out;
    while (getline(&line, &lcap, stdin) > 0) {
        ++lineno;
        tok.clear();
        for (char* t = strtok(line, " \n"); t; t = strtok(nullptr, " \n"))
            tok.push_back(t);
        if (tok.empty()) continue;
        auto it = sigs.find(tok[0]);
        if (it == sigs.end() || tok.size() != 4 + it->second.size()) {
            printf("BADCASE line %lld\n", lineno);
            return 2;
        }
        const std::string& op = tok[0];
        const std::string& sig = it->second;
        ++counts[op];
        int shift = atoi(tok[1].c_str());
        int pad = atoi(tok[2].c_str());
        unsigned long long cap = strtoull(tok[3].c_str(), nullptr, 10);
        if (shift < 0 || shift > 7 || cap > HEAP_MAX) {
            printf("BADCASE line %lld\n", lineno);
            return 2;
        }

        // ---- subject arena -------------------------------------------------
        std::vector<std::string> sv;
        std::vector<long long> iv;
        std::vector<double> dv;
        for (size_t k = 0; k < sig.size(); ++k) {
            const std::string& t = tok[4 + k];
            if (sig[k] == 's') sv.push_back(unhex(t));
            else if (sig[k] == 'i') iv.push_back(strtoll(t.c_str(), nullptr, 10));
            else dv.push_back(get_d(t));
        }
        size_t pos = 64 + shift;
        std::vector<size_t> offs;
        for (auto& s : sv) {
            offs.push_back(pos);
            pos = ((pos + s.size() + 16 + 7) & ~(size_t)7) + shift;
        }
        size_t asize = sv.empty() ? 96
                                  : offs.back() + sv.back().size() + 16;
        char* arena = (char*)malloc(asize);
        memset(arena, pad, asize);
        std::vector<tstr> S;
        for (size_t k = 0; k < sv.size(); ++k) {
            memcpy(arena + offs[k], sv[k].data(), sv[k].size());
            S.push_back(tstr{arena + offs[k], (long long)sv[k].size()});
        }
        char* shadow = (char*)malloc(asize);
        memcpy(shadow, arena, asize);

        // ---- heap ----------------------------------------------------------
        unsigned long long cursor = 0;
        TpxHeap h{hb, &cursor, cap, nullptr, nullptr};

        int ec = 0;
        const char* bad = nullptr;
        out.clear();
        const char* rp = nullptr;   // result range, when it is a string
        long long rn = 0;
        bool loose = false;         // result is not the only heap content
        auto str_result = [&](tstr r) {
            rp = r.p; rn = r.n;
            if (!ec) put_hex(out, r.p, r.n);
        };

        if (op == "memchr") {
            put_i(out, tpx_memchr(S[0].p, S[0].n, (char)iv[0]));
        } else if (op == "memchr_hi") {
            unsigned long long hi = 0;
            put_i(out, tpx_memchr_hi(S[0].p, S[0].n, (char)iv[0], &hi));
            out += hi ? " 1" : " 0";
            if (hi & ~TPX_SWAR_HIGH) out += " HIBITS";
        } else if (op == "memchr2") {
            put_i(out, tpx_memchr2(S[0].p, S[0].n, (char)iv[0], (char)iv[1]));
        } else if (op == "memrchr") {
            put_i(out, tpx_memrchr(S[0].p, S[0].n, (char)iv[0]));
        } else if (op == "memchr_hi_spec") {
            unsigned long long hi = 0;
            int spec = 0;
            put_i(out, tpx_memchr_hi_spec(S[0].p, S[0].n, (char)iv[0], &hi,
                                          (int)iv[1], &spec));
            out += hi ? " 1" : " 0";
            out += spec ? " 1" : " 0";
        } else if (op == "ascii") {
            put_i(out, tpx_ascii(S[0]) ? 1 : 0);
        } else if (op == "csv_needs_quote") {
            long long q = -1;
            bool need = tpx_csv_needs_quote(S[0], &q);
            put_i(out, need ? 1 : 0); out += " "; put_i(out, q);
        } else if (op == "csv_cell_len") {
            put_i(out, tpx_csv_cell_len(S[0]));
        } else if (op == "csv_cell_write") {
            long long len = tpx_csv_cell_len(S[0]);
            char* w = tpx_alloc(h, len);
            if (!w) ec = EC_MEMORYERROR;
            else {
                char* e = tpx_csv_cell_write(w, S[0]);
                if (e - w != len) out += "LENMISMATCH ";
                str_result(tstr{w, len});
            }
        } else if (op == "memcpy") {
            // dest at every alignment too: iv[0] = 0..7 bytes into the alloc
            long long n = S[0].n;
            char* w = tpx_alloc(h, n + 8);
            if (!w) ec = EC_MEMORYERROR;
            else {
                tpx_memcpy(w + iv[0], S[0].p, n);
                str_result(tstr{w + iv[0], n});
            }
        } else if (op == "find") {
            put_i(out, tpx_find(S[0], S[1], &ec));
        } else if (op == "rfind") {
            put_i(out, tpx_rfind(S[0], S[1], &ec));
        } else if (op == "contains") {
            put_i(out, tpx_contains(S[0], S[1]) ? 1 : 0);
        } else if (op == "startswith") {
            put_i(out, tpx_startswith(S[0], S[1]) ? 1 : 0);
        } else if (op == "endswith") {
            put_i(out, tpx_endswith(S[0], S[1]) ? 1 : 0);
        } else if (op == "streq") {
            put_i(out, tpx_streq(S[0], S[1]) ? 1 : 0);
        } else if (op == "strcmp") {
            put_i(out, tpx_strcmp(S[0], S[1]));
        } else if (op == "getitem") {
            str_result(tpx_getitem(S[0], iv[0], &ec));
        } else if (op == "slice") {
            str_result(tpx_slice(S[0], iv[0], iv[1] != 0, iv[2], iv[3] != 0,
                                 &ec));
        } else if (op == "center") {
            str_result(tpx_center(h, S[0], iv[0], S[1], &ec));
        } else if (op == "strmul") {
            str_result(tpx_strmul(h, S[0], iv[0], &ec));
            // a repeat that cannot exist is rejected before any allocation
            if (S[0].n > 0 && iv[0] > 0 && cursor != 0 &&
                (unsigned long long)iv[0] > cap / (unsigned long long)S[0].n)
                bad = "rejected repeat still allocated";
        } else if (op == "lower") {
            str_result(tpx_lower(h, S[0], &ec));
        } else if (op == "upper") {
            str_result(tpx_upper(h, S[0], &ec));
        } else if (op == "swapcase") {
            str_result(tpx_swapcase(h, S[0], &ec));
        } else if (op == "capitalize_ix") {
            str_result(tpx_capitalize_ix(h, S[0], &ec));
        } else if (op == "strip") {
            str_result(tpx_strip(S[0], &ec));
        } else if (op == "concat") {
            str_result(tpx_concat(h, S[0], S[1], &ec));
        } else if (op == "replace") {
            str_result(tpx_replace(h, S[0], S[1], S[2], &ec));
        } else if (op == "splitget") {
            str_result(tpx_splitget(S[0], S[1], iv[0], &ec));
        } else if (op == "int_drop") {
            loose = true;  // the >31 B path leaves replace()'s copy in the heap
            long long v = tpx_int_drop(h, S[0], S[1].p[0], S[1], &ec);
            put_i(out, v);
        } else if (op == "atoi") {
            long long v = 0;
            int rc = tpx_fast_atoi64(S[0].p, S[0].p + S[0].n, &v);
            put_i(out, rc); if (!rc) { out += " "; put_i(out, v); }
        } else if (op == "atod") {
            double v = 0;
            int rc = tpx_fast_atod(S[0].p, S[0].p + S[0].n, &v);
            put_i(out, rc); if (!rc) { out += " "; put_d(out, v); }
        } else if (op == "int_str") {
            put_i(out, tpx_int_str(S[0], &ec));
        } else if (op == "float_str") {
            put_d(out, tpx_float_str(S[0], &ec));
        } else if (op == "cell_i64") {
            tpx_cell c{S[0].p, S[0].n, 0};
            long long v = 0;
            int rc = tpx_cell_i64(c, &v);
            put_i(out, rc); if (!rc) { out += " "; put_i(out, v); }
        } else if (op == "cell_f64") {
            tpx_cell c{S[0].p, S[0].n, 0};
            double v = 0;
            int rc = tpx_cell_f64(c, &v);
            put_i(out, rc); if (!rc) { out += " "; put_d(out, v); }
        } else if (op == "cell_bool") {
            tpx_cell c{S[0].p, S[0].n, 0};
            bool v = false;
            int rc = tpx_cell_bool(c, &v);
            put_i(out, rc); if (!rc) { out += " "; put_i(out, v ? 1 : 0); }
        } else if (op == "floordiv_i64") {
            put_i(out, tpx_floordiv_i64(iv[0], iv[1], &ec));
        } else if (op == "mod_i64") {
            put_i(out, tpx_mod_i64(iv[0], iv[1], &ec));
        } else if (op == "truediv") {
            put_d(out, tpx_truediv(dv[0], dv[1], &ec));
        } else if (op == "floordiv_f64") {
            put_d(out, tpx_floordiv_f64(dv[0], dv[1], &ec));
        } else if (op == "mod_f64") {
            put_d(out, tpx_mod_f64(dv[0], dv[1], &ec));
        } else if (op == "int_f64") {
            put_i(out, tpx_int_f64(dv[0], &ec));
        } else if (op == "i64_digits") {
            put_i(out, tpx_i64_digits(iv[0]));
        } else if (op == "i64_write") {
            long long len = tpx_i64_digits(iv[0]);
            char* w = tpx_alloc(h, len);
            if (!w) ec = EC_MEMORYERROR;
            else { tpx_i64_write(w, iv[0], len); str_result(tstr{w, len}); }
        } else if (op == "str_i64") {
            str_result(tpx_str_i64(h, iv[0], &ec));
        } else if (op == "fmt0d") {
            str_result(tpx_fmt0d(h, iv[0], iv[1], &ec));
        } else if (op == "f64_csv") {
            unsigned long long N = 0;
            bool neg = false;
            int rc = tpx_f64_csv_n(dv[0], &N, &neg);
            put_i(out, rc);
            if (!rc) {
                long long len = tpx_f64_csv_len(N, neg);
                out += " "; put_i(out, len); out += " ";
                char* w = tpx_alloc(h, len > 0 ? len : 1);
                if (!w) ec = EC_MEMORYERROR;
                else {
                    char* e = tpx_f64_csv_write(w, N, neg);
                    str_result(tstr{w, (long long)(e - w)});
                }
            }
        } else if (op == "csv_row") {
            // byte walk over one (newline-stripped) row until no cell follows:
            // "<hi> <flags&6 OR> <ncells> <cell>..."
            const char* cur = S[0].p;
            const char* end = S[0].p + S[0].n;
            unsigned long long hi = 0;
            int fl = 0;
            long long nc = 0;
            std::string cells;
            bool more = true;
            while (more) {
                tpx_cell c;
                cur = tpx_csv_next_cell(cur, end, &c, &more, (char)iv[0], &hi);
                fl |= c.flags & 6;
                ++nc;
                cells += " ";
                put_hex(cells, c.p, c.n);
                if (nc > S[0].n + 2) { cells += " RUNAWAY"; break; }
            }
            out += hi ? "1 " : "0 ";
            put_i(out, fl); out += " "; put_i(out, nc); out += cells;
        }

        // ---- memory contract -----------------------------------------------
        if (memcmp(arena, shadow, asize) != 0) bad = "arena written";
        if (memcmp(heapbuf, canary, GUARD) != 0) bad = "write before heap";
        unsigned long long used = cursor < cap ? cursor : cap;
        // an error code means nothing was produced (int_drop may raise its
        // ValueError after replace() wrote its copy)
        if (ec == EC_MEMORYERROR || (ec && !loose)) used = 0;
        if (memcmp(hb + used, canary, HEAP_MAX - used + GUARD) != 0)
            bad = used ? "write past heap cursor"
                       : "heap written despite error code";
        if (!bad && !ec && !loose && used) {
            long long a = 0, b = 0;  // result range inside the heap, if any
            if (rp >= hb && rp < hb + HEAP_MAX && rn > 0) {
                a = rp - hb; b = a + rn;
                if ((unsigned long long)b > used) bad = "result past cursor";
            }
            if (!bad && (memcmp(hb, canary, a) != 0 ||
                         memcmp(hb + b, canary, used - b) != 0))
                bad = "heap written outside the result";
        }
        if (bad) printf("MEMFAIL %s\n", bad);
        else if (ec) printf("E%d\n", ec);
        else printf("%s\n", out.c_str());

        if (cursor || bad) memset(heapbuf, CANARY, GUARD + HEAP_MAX + GUARD);
        free(shadow);
        free(arena);
    }
    for (auto& kv : counts)
        fprintf(stderr, "%-16s %lld\n", kv.first.c_str(), kv.second);
    for (auto& s : SIGS)
        if (!counts.count(s[0])) fprintf(stderr, "%-16s 0\n", s[0]);
    printf("OK\n");
    free(line);
    free(heapbuf);
    free(canary);
    return 0;
}
