// Host-compiled driver for the string builders of csrc/tpx_fmt.hip.h
// (tpx_format, tpx_capwords). tests/test_host_fmt.py writes one request per
// line, this program answers one line each, and the Python side compares with
// what CPython computes. Built plain and with ASan+UBSan; the same host shims
// as tests/host_rt_test.cpp (TPX_HOST_TEST strips the device-only kernels).
//
// request:  F <cap> <align> <nitems> <w0,w1,..> <blobhex|-> <nargs> {I <int> | S <hex|->}..
//           C <cap> <align> <hex|->
// answer:   <ec> <resulthex|-> <heap bytes used> <clean>
//   cap    heap capacity in bytes
//   align  0..7: every source string starts at an 8-aligned address + align
//   clean  1 when the canaries around the heap are intact and, on an error,
//          no heap byte changed
#define TPX_HOST_TEST 1
#define __HIPRTC__ 1
#define __device__
#define __forceinline__ inline
#define __noinline__ __attribute__((noinline))
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
static inline long long __double_as_longlong(double d) {
    long long v; memcpy(&v, &d, 8); return v;
}
static inline double __longlong_as_double(long long v) {
    double d; memcpy(&d, &v, 8); return d;
}

#include "../tuplex_amd/csrc/tpx_rt.hip.h"
#include "../tuplex_amd/csrc/tpx_fmt.hip.h"

#define PAD 16          // tpx_memcpy may read the aligned words around a source
#define CANARY 32
#define FILL 0xA5

static std::string unhex(const char* h) {
    std::string out;
    if (h[0] == '-') return out;
    for (size_t i = 0; h[i] && h[i + 1]; i += 2) {
        unsigned v;
        sscanf(h + i, "%2x", &v);
        out.push_back((char)v);
    }
    return out;
}

// a copy of `s` at an 8-aligned address + align, PAD bytes on both sides
struct Placed {
    char* raw;
    char* p;
    Placed(const std::string& s, int align) {
        raw = (char*)malloc(s.size() + 2 * PAD + 16);
        memset(raw, '#', s.size() + 2 * PAD + 16);
        uintptr_t a = ((uintptr_t)raw + PAD + 7) & ~(uintptr_t)7;
        p = (char*)a + align;
        memcpy(p, s.data(), s.size());
    }
    Placed(const Placed&) = delete;
    ~Placed() { free(raw); }
};

struct Heap {
    std::vector<unsigned char> buf;
    unsigned long long cursor;
    TpxHeap h;
    explicit Heap(long long cap) : buf((size_t)cap + 2 * CANARY + 8, FILL), cursor(0) {
        uintptr_t a = ((uintptr_t)buf.data() + CANARY + 7) & ~(uintptr_t)7;
        h.base = (char*)a;
        h.cursor = &cursor;
        h.cap = (unsigned long long)cap;
        h.tl_cur = nullptr;
        h.tl_end = nullptr;
    }
    bool canaries_ok() const {
        const unsigned char* lo = (const unsigned char*)h.base;
        const unsigned char* hi = lo + h.cap;
        for (const unsigned char* q = buf.data(); q < lo; ++q)
            if (*q != FILL) return false;
        for (const unsigned char* q = hi; q < buf.data() + buf.size(); ++q)
            if (*q != FILL) return false;
        return true;
    }
    bool untouched() const {
        for (unsigned long long i = 0; i < h.cap; ++i)
            if ((unsigned char)h.base[i] != FILL) return false;
        return true;
    }
};

static void answer(const Heap& hp, int ec, tstr r) {
    bool clean = hp.canaries_ok() && (ec == 0 || hp.untouched());
    printf("%d ", ec);
    if (ec != 0 || r.n == 0) {
        printf("-");
    } else {
        for (long long i = 0; i < r.n; ++i)
            printf("%02x", (unsigned)(unsigned char)r.p[i]);
    }
    printf(" %llu %d\n", hp.cursor, clean ? 1 : 0);
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s requests\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror("open"); return 2; }
    std::vector<char> line(1 << 16);
    while (fgets(line.data(), (int)line.size(), f)) {
        std::vector<char*> tok;
        for (char* t = strtok(line.data(), " \n"); t; t = strtok(nullptr, " \n"))
            tok.push_back(t);
        if (tok.empty()) continue;
        long long cap = atoll(tok[1]);
        int align = atoi(tok[2]);
        Heap hp(cap);
        int ec = 0;
        if (tok[0][0] == 'C') {
            std::string s = unhex(tok[3]);
            Placed ps(s, align);
            tstr r = tpx_capwords(hp.h, tstr{ps.p, (long long)s.size()}, &ec);
            answer(hp, ec, r);
            continue;
        }
        int nitems = atoi(tok[3]);
        std::vector<int> words;
        for (char* w = strtok(tok[4], ","); w; w = strtok(nullptr, ","))
            words.push_back(atoi(w));
        if ((int)words.size() != nitems * TPX_FMT_WORDS) {
            fprintf(stderr, "bad request: %d items, %zu words\n", nitems,
                    words.size());
            return 2;
        }
        std::string blob = unhex(tok[5]);
        Placed pblob(blob, align);
        int nargs = atoi(tok[6]);
        std::vector<TpxFmtArg> args((size_t)nargs + 1);
        std::vector<Placed*> keep;
        for (int k = 0; k < nargs; ++k) {
            const char* kind = tok[7 + 2 * k];
            const char* val = tok[8 + 2 * k];
            if (kind[0] == 'I') {
                args[k].p = nullptr;
                args[k].n = strtoll(val, nullptr, 10);
            } else {
                std::string s = unhex(val);
                Placed* ps = new Placed(s, align);
                keep.push_back(ps);
                args[k].p = ps->p;
                args[k].n = (long long)s.size();
            }
        }
        tstr r = tpx_format(hp.h, words.data(), nitems, pblob.p, args.data(),
                            &ec);
        answer(hp, ec, r);
        for (Placed* ps : keep) delete ps;
    }
    fclose(f);
    printf("DONE\n");
    return 0;
}
