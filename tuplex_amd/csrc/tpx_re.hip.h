// tpx_re.hip.h — per-thread backtracking regex VM for compiled re.search /
// re.match / re.fullmatch UDF calls (gfx950).
//
// The reference compiles constant-pattern re.search calls against pcre2
// (codegen/src/FunctionRegistry.cc). Here tuplex_amd/udf/relower.py lowers the
// pattern, parsed by CPython's own sre parser, to the word program below and
// codegen.py embeds it as a `__device__ const int` array next to the stage's
// string literals. One thread runs one subject string; priority order is
// CPython's (leftmost start, alternatives in order, greedy/lazy as written).
//
// Appended after tpx_rt.hip.h ONLY in stages that contain a regex call, so the
// source (and the hsaco cache key) of every other stage is unchanged.
//
// Bounded work: a fixed explicit stack in private memory and a step budget
// TPX_RE_BUDGET_A + TPX_RE_BUDGET_B * len(s). Exhausting either sets EC_NCV:
// the row takes the silent host replay (CPython computes the exact answer),
// exactly like a row with a non-ASCII byte. A byte >= 0x80 under a character
// class or \b diverts the same way (class membership is a 128-bit ASCII map;
// CPython's unicode categories decide those rows). The limits therefore never
// change a result, only where it is computed.
//
// Observed maxima over the well-formed Common-Log fixture
// (tests/regex_pipelines.py, ten patterns x 4900 lines; tests/test_host_re.py
// asserts they stay within a quarter of the limits):
//   steps  max 217 on a 119-byte line  (limit 512 + 16*119 = 2416; ratio 0.09)
//   stack  max 5 frames                (limit 32; one frame per span or
//                                       alternative, not per character)
#pragma once

#define TPX_RE_STACK 32       // backtrack frames (3 ints each, private memory)
#define TPX_RE_BUDGET_A 512   // step budget = A + B * len(subject)
#define TPX_RE_BUDGET_B 16

// program header words
#define TPX_RE_H_NCAPS 0      // 2 * (ngroups + 1)
#define TPX_RE_H_FLAGS 1      // bit0: try start position 0 only
#define TPX_RE_H_FIRST 2      // literal first byte of every match, or -1
#define TPX_RE_H_LEN 3        // total words (host-side validation)
#define TPX_RE_H_SIZE 4

// opcodes: [op, operands...]
#define TPX_RE_CHAR 1         // c
#define TPX_RE_LIT 2          // n, ceil(n/4) words of packed bytes (LE)
#define TPX_RE_CLASS 3        // b0 b1 b2 b3 (128-bit ASCII bitmap)
#define TPX_RE_SPAN 4         // min max flags b0 b1 b2 b3
#define TPX_RE_SPLIT 5        // pc_first pc_second
#define TPX_RE_JMP 6          // pc
#define TPX_RE_SAVE 7         // k          (group on every match path)
#define TPX_RE_SAVER 8        // k          (optional group: restored on backtrack)
#define TPX_RE_ASSERT 9       // kind b0 b1 b2 b3 (bitmap: \w, for \b \B)
#define TPX_RE_MATCH 10

#define TPX_RE_SPAN_WORDS 8
#define TPX_RE_SPAN_LAZY 1
#define TPX_RE_SPAN_NOBT 2    // greedy, and shrinking can never help: no frame
#define TPX_RE_SPAN_INF 0x7fffffff

#define TPX_RE_AT_BOS 0       // ^ \A (no MULTILINE)
#define TPX_RE_AT_EOL 1       // $  : end, or before one trailing \n
#define TPX_RE_AT_EOS 2       // \Z : true end
#define TPX_RE_AT_WB 3        // \b
#define TPX_RE_AT_NWB 4       // \B
#define TPX_RE_AT_NWB_E 5     // \B that also matches the empty subject

// frame kinds (high byte of word 0; low 24 bits: pc or capture index)
#define TPX_RE_F_ALT 0        // [pc, pos, -]        resume at pc
#define TPX_RE_F_GSPAN 1      // [pc, start, end]    shrink end by one
#define TPX_RE_F_LSPAN 2      // [pc, start, end]    grow end by one
#define TPX_RE_F_CAP 3        // [k, old value, -]   restore caps[k]

__device__ __forceinline__ bool tpx_re_in(unsigned long long lo,
                                          unsigned long long hi, unsigned c) {
    return ((((c & 64u) ? hi : lo) >> (c & 63u)) & 1ULL) != 0;
}

__device__ __forceinline__ unsigned long long tpx_re_u64(int a, int b) {
    return (unsigned long long)(unsigned)a |
           ((unsigned long long)(unsigned)b << 32);
}

// Runs `prog` over s. On a match returns true with caps[2k], caps[2k+1] the
// byte span of group k (-1, -1: group did not take part). On a divert sets
// *ec = EC_NCV and returns false. stats (nullable): [steps, peak frames].
// Out of line on purpose: inlined into both row bodies of tpx_stage_main the
// nine-group logs stage took 255 VGPRs (137 this way) and ran no faster
// (profiles/README.md).
__device__ __attribute__((noinline)) bool tpx_re_run(
    const int* prog, const tstr s, int* caps, int* ec, int* stats) {
    const int ncaps = prog[TPX_RE_H_NCAPS];
    const int hflags = prog[TPX_RE_H_FLAGS];
    const int first = prog[TPX_RE_H_FIRST];
    const char* p = s.p;
    if (s.n > 0x3fffffffLL) { *ec = EC_NCV; return false; }
    const int n = (int)s.n;
    const long long budget =
        TPX_RE_BUDGET_A + (long long)TPX_RE_BUDGET_B * (long long)n;
    int stk[TPX_RE_STACK * 3];
    long long steps = 0;
    int peak = 0;
    bool divert = false, matched = false;

    for (int start = 0; start <= n && !divert && !matched; ++start) {
        if (first >= 0) {
            long long k = tpx_memchr(p + start, (long long)(n - start),
                                     (char)first);
            if (k < 0) break;
            start += (int)k;
            steps += k >> 4;
        }
        for (int i = 0; i < ncaps; ++i) caps[i] = -1;
        caps[0] = start;
        int sp = 0, pc = TPX_RE_H_SIZE, pos = start;
        bool fail = false;
        for (;;) {
            if (++steps > budget) { divert = true; break; }
            if (fail) {
                if (sp == 0) break;  // no alternative left at this start
                int* f = stk + (sp - 1) * 3;
                const int kind = (int)((unsigned)f[0] >> 24);
                const int fpc = f[0] & 0xffffff;
                if (kind == TPX_RE_F_ALT) {
                    pc = fpc; pos = f[1]; --sp; fail = false;
                } else if (kind == TPX_RE_F_CAP) {
                    caps[fpc] = f[1]; --sp;
                } else if (kind == TPX_RE_F_GSPAN) {
                    const int mn = prog[fpc + 1];
                    const int e = f[2] - 1;  // frame exists only if end > start+min
                    pos = e; pc = fpc + TPX_RE_SPAN_WORDS; fail = false;
                    if (e - f[1] <= mn) --sp; else f[2] = e;
                } else {  // TPX_RE_F_LSPAN
                    const int mx = prog[fpc + 2];
                    const int e = f[2];
                    bool ok = e < n && (mx == TPX_RE_SPAN_INF || e - f[1] < mx);
                    if (ok) {
                        const unsigned c = (unsigned char)p[e];
                        if (c >= 128u) { divert = true; break; }
                        ok = tpx_re_in(tpx_re_u64(prog[fpc + 4], prog[fpc + 5]),
                                       tpx_re_u64(prog[fpc + 6], prog[fpc + 7]), c);
                    }
                    if (ok) {
                        f[2] = e + 1; pos = e + 1;
                        pc = fpc + TPX_RE_SPAN_WORDS; fail = false;
                    } else {
                        --sp;
                    }
                }
                continue;
            }
            const int op = prog[pc];
            if (op == TPX_RE_CHAR) {
                if (pos < n && (unsigned char)p[pos] == (unsigned)prog[pc + 1]) {
                    ++pos; pc += 2;
                } else fail = true;
            } else if (op == TPX_RE_LIT) {
                const int ln = prog[pc + 1];
                if (n - pos < ln) { fail = true; continue; }
                bool eq = true;
                for (int i = 0; i < ln && eq; ++i) {
                    const unsigned w = (unsigned)prog[pc + 2 + (i >> 2)];
                    eq = (unsigned char)p[pos + i] == ((w >> ((i & 3) * 8)) & 255u);
                }
                if (eq) { pos += ln; pc += 2 + ((ln + 3) >> 2); } else fail = true;
            } else if (op == TPX_RE_CLASS) {
                if (pos >= n) { fail = true; continue; }
                const unsigned c = (unsigned char)p[pos];
                if (c >= 128u) { divert = true; break; }
                if (tpx_re_in(tpx_re_u64(prog[pc + 1], prog[pc + 2]),
                              tpx_re_u64(prog[pc + 3], prog[pc + 4]), c)) {
                    ++pos; pc += 5;
                } else fail = true;
            } else if (op == TPX_RE_SPAN) {
                const int mn = prog[pc + 1], mx = prog[pc + 2];
                const int fl = prog[pc + 3];
                const unsigned long long lo = tpx_re_u64(prog[pc + 4], prog[pc + 5]);
                const unsigned long long hi = tpx_re_u64(prog[pc + 6], prog[pc + 7]);
                const int room = n - pos;
                // lazy: take the minimum now, grow on backtrack
                const int want = (fl & TPX_RE_SPAN_LAZY) ? mn
                                 : (mx == TPX_RE_SPAN_INF || mx > room ? room : mx);
                if (mn > room) { fail = true; continue; }
                int e = pos;
                const int lim = pos + want;
                bool hib = false;
                while (e < lim) {
                    const unsigned c = (unsigned char)p[e];
                    if (c >= 128u) { hib = true; break; }
                    if (!tpx_re_in(lo, hi, c)) break;
                    ++e;
                }
                if (hib) { divert = true; break; }
                steps += (e - pos) >> 4;
                if (e - pos < mn) { fail = true; continue; }
                const bool lazy = (fl & TPX_RE_SPAN_LAZY) != 0;
                const bool need = lazy ? (mx == TPX_RE_SPAN_INF || mn < mx)
                                       : (e - pos > mn && !(fl & TPX_RE_SPAN_NOBT));
                if (need) {
                    if (sp >= TPX_RE_STACK) { divert = true; break; }
                    int* f = stk + sp * 3;
                    f[0] = ((lazy ? TPX_RE_F_LSPAN : TPX_RE_F_GSPAN) << 24) | pc;
                    f[1] = pos; f[2] = e;
                    ++sp; if (sp > peak) peak = sp;
                }
                pos = e; pc += TPX_RE_SPAN_WORDS;
            } else if (op == TPX_RE_SPLIT) {
                if (sp >= TPX_RE_STACK) { divert = true; break; }
                int* f = stk + sp * 3;
                f[0] = (TPX_RE_F_ALT << 24) | prog[pc + 2];
                f[1] = pos; f[2] = 0;
                ++sp; if (sp > peak) peak = sp;
                pc = prog[pc + 1];
            } else if (op == TPX_RE_JMP) {
                pc = prog[pc + 1];
            } else if (op == TPX_RE_SAVE) {
                caps[prog[pc + 1]] = pos; pc += 2;
            } else if (op == TPX_RE_SAVER) {
                if (sp >= TPX_RE_STACK) { divert = true; break; }
                const int k = prog[pc + 1];
                int* f = stk + sp * 3;
                f[0] = (TPX_RE_F_CAP << 24) | k;
                f[1] = caps[k]; f[2] = 0;
                ++sp; if (sp > peak) peak = sp;
                caps[k] = pos; pc += 2;
            } else if (op == TPX_RE_ASSERT) {
                const int kind = prog[pc + 1];
                bool ok;
                if (kind == TPX_RE_AT_BOS) {
                    ok = pos == 0;
                } else if (kind == TPX_RE_AT_EOL) {
                    ok = pos == n || (pos == n - 1 && p[pos] == '\n');
                } else if (kind == TPX_RE_AT_EOS) {
                    ok = pos == n;
                } else if (n == 0) {
                    // \b never matches the empty subject; whether \B does
                    // depends on the CPython version: the lowering asked it
                    ok = kind == TPX_RE_AT_NWB_E;
                } else {
                    const unsigned long long lo = tpx_re_u64(prog[pc + 2], prog[pc + 3]);
                    const unsigned long long hi = tpx_re_u64(prog[pc + 4], prog[pc + 5]);
                    const unsigned a = pos > 0 ? (unsigned char)p[pos - 1] : 0u;
                    const unsigned b = pos < n ? (unsigned char)p[pos] : 0u;
                    if ((a | b) >= 128u) { divert = true; break; }
                    const bool wa = pos > 0 && tpx_re_in(lo, hi, a);
                    const bool wb = pos < n && tpx_re_in(lo, hi, b);
                    ok = (kind == TPX_RE_AT_WB) ? (wa != wb) : (wa == wb);
                }
                if (ok) pc += 6; else fail = true;
            } else {  // TPX_RE_MATCH
                caps[1] = pos; matched = true; break;
            }
        }
        if (hflags & 1) break;
    }
    if (stats) { stats[0] = (int)steps; stats[1] = peak; }
    if (divert) { *ec = EC_NCV; return false; }
    return matched;
}

__device__ __forceinline__ bool tpx_re_exec(const int* prog, const tstr s,
                                            int* caps, int* ec) {
    return tpx_re_run(prog, s, caps, ec, nullptr);
}

// group k of a successful match as a view into the subject
__device__ __forceinline__ tstr tpx_re_group(const tstr s, const int* caps,
                                             int k) {
    const int a = caps[2 * k], b = caps[2 * k + 1];
    if (a < 0 || b < a) return tstr{s.p, 0};
    return tstr{s.p + a, (long long)(b - a)};
}
