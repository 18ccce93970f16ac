// Host-compiled driver for the device regex VM (tuplex_amd/csrc/tpx_re.hip.h),
// used by tests/test_host_re.py: the VM's group spans must equal CPython's on
// fuzzed patterns/subjects. Same TPX_HOST_TEST macro set as host_rt_test.cpp.
//
// stdin:   P <nwords> <w0> <w1> ...     select a program
//          S <hex bytes or '-'>         run it over a subject
// stdout:  one line per S: <divert> <matched> <steps> <peak> <a0> <b0> <a1> ...
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
static inline long long __double_as_longlong(double d) {
    long long v; memcpy(&v, &d, 8); return v;
}
static inline double __longlong_as_double(long long v) {
    double d; memcpy(&d, &v, 8); return d;
}

#include "../tuplex_amd/csrc/tpx_rt.hip.h"
#include "../tuplex_amd/csrc/tpx_re.hip.h"

static int hexv(int c) {
    if (c >= '0' && c <= '9') return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    return -1;
}

int main(void) {
    std::vector<int> prog;
    std::string line;
    std::vector<char> buf;
    int ch;
    for (;;) {
        line.clear();
        while ((ch = getchar()) != EOF && ch != '\n') line.push_back((char)ch);
        if (line.empty() && ch == EOF) break;
        if (line.empty()) continue;
        if (line[0] == 'P') {
            prog.clear();
            char* q = &line[1];
            long nw = strtol(q, &q, 10);
            for (long i = 0; i < nw; ++i) prog.push_back((int)strtol(q, &q, 10));
            if ((long)prog.size() != nw || nw < TPX_RE_H_SIZE + 1 ||
                prog[TPX_RE_H_LEN] != nw) {
                fprintf(stderr, "bad program line\n");
                return 2;
            }
        } else if (line[0] == 'S') {
            if (prog.empty()) { fprintf(stderr, "S before P\n"); return 2; }
            // exact-size heap copy: ASan sees any read past the subject
            std::vector<char> subj;
            size_t i = 2;
            while (i + 1 < line.size() && hexv(line[i]) >= 0 &&
                   hexv(line[i + 1]) >= 0) {
                subj.push_back((char)(hexv(line[i]) * 16 + hexv(line[i + 1])));
                i += 2;
            }
            char* sp = (char*)malloc(subj.size() ? subj.size() : 1);
            if (!subj.empty()) memcpy(sp, subj.data(), subj.size());
            int ncaps = prog[TPX_RE_H_NCAPS];
            std::vector<int> caps((size_t)ncaps, -7);
            int ec = 0, stats[2] = {0, 0};
            bool m = tpx_re_run(prog.data(), tstr{sp, (long long)subj.size()},
                                caps.data(), &ec, stats);
            printf("%d %d %d %d", ec == EC_NCV ? 1 : 0, m ? 1 : 0, stats[0],
                   stats[1]);
            if (m)
                for (int k = 0; k < ncaps; ++k) printf(" %d", caps[(size_t)k]);
            printf("\n");
            free(sp);
        }
    }
    printf("OK\n");
    return 0;
}
