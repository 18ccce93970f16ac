// tpx_fmt.hip.h — single-allocation string builders for compiled str.format /
// multi-directive '%' / string.capwords UDF calls (gfx950).
//
// tuplex_amd/udf/fmtspec.py parses the constant template into items;
// codegen.py embeds them as a `__device__ const int` array (four words per
// item) plus one byte blob of all literal segments, next to the stage's
// string literals. Both builders run two passes over their input: the exact
// output length first, then ONE tpx_alloc, then the bytes left to right. When
// the heap is exhausted they raise EC_MEMORYERROR before any byte is written.
//
// Appended after tpx_rt.hip.h ONLY in stages that contain a format or capwords
// node, so the source (and the hsaco cache key) of every other stage is
// unchanged.
//
// Width counts characters: a str field WITH a width on a value that holds a
// byte >= 0x80 sets EC_NCV (silent host replay, CPython pads it); without a
// width the bytes are copied as they are. capwords diverts on any byte >= 0x80
// (unicode whitespace and case rules decide those rows).
#pragma once

// Both builders are real calls, not inlined: a stage calls them from several
// branches of its row body, and the out-of-line form left tpx_stage_main with
// fewer VGPRs than the inlined one (profiles/README.md has both counts). The
// argument array then lives in the private segment.
#ifndef TPX_FMT_FN
#define TPX_FMT_FN __device__ __noinline__
#endif

#define TPX_FMT_LIT 0    // [0, blob offset, length, 0]
#define TPX_FMT_INT 1    // [1, arg, flags, width]
#define TPX_FMT_STR 2    // [2, arg, flags, width]
#define TPX_FMT_WORDS 4
#define TPX_FMT_ZERO 1   // pad with zeros after the sign
#define TPX_FMT_LEFT 2   // pad on the right

// one format argument: a str view, or an i64 in n (p unused)
struct TpxFmtArg {
    const char* p;
    long long n;
};

__device__ __forceinline__ long long tpx_fmt_max(long long a, long long b) {
    return a < b ? b : a;
}

TPX_FMT_FN tstr tpx_format(TpxHeap& h, const int* prog, int nitems,
                           const char* lits, const TpxFmtArg* args, int* ec) {
    long long total = 0;
    for (int k = 0; k < nitems; ++k) {
        const int* it = prog + TPX_FMT_WORDS * k;
        if (it[0] == TPX_FMT_LIT) {
            total += it[2];
        } else if (it[0] == TPX_FMT_INT) {
            total += tpx_fmt_max(tpx_i64_digits(args[it[1]].n), it[3]);
        } else {
            const tstr s = tstr{args[it[1]].p, args[it[1]].n};
            if (it[3] > 0 && !tpx_ascii(s)) {
                *ec = EC_NCV;
                return tstr{lits, 0};
            }
            total += tpx_fmt_max(s.n, it[3]);
        }
    }
    char* d = tpx_alloc(h, total);
    if (!d) { *ec = EC_MEMORYERROR; return tstr{lits, 0}; }
    char* w = d;
    for (int k = 0; k < nitems; ++k) {
        const int* it = prog + TPX_FMT_WORDS * k;
        if (it[0] == TPX_FMT_LIT) {
            tpx_memcpy(w, lits + it[1], it[2]);
            w += it[2];
        } else if (it[0] == TPX_FMT_INT) {
            const long long v = args[it[1]].n;
            const long long dl = tpx_i64_digits(v);
            const long long pad = tpx_fmt_max(dl, it[3]) - dl;
            if (it[2] & TPX_FMT_LEFT) {
                tpx_i64_write(w, v, dl);
                for (long long i = 0; i < pad; ++i) w[dl + i] = ' ';
            } else if (it[2] & TPX_FMT_ZERO) {
                for (long long i = 0; i < pad; ++i) w[i] = '0';
                tpx_i64_write(w + pad, v, dl);
                if (v < 0 && pad > 0) {  // sign before the zeros: '-05'
                    w[pad] = '0';
                    w[0] = '-';
                }
            } else {
                for (long long i = 0; i < pad; ++i) w[i] = ' ';
                tpx_i64_write(w + pad, v, dl);
            }
            w += dl + pad;
        } else {
            const tstr s = tstr{args[it[1]].p, args[it[1]].n};
            const long long pad = tpx_fmt_max(s.n, it[3]) - s.n;
            if (it[2] & TPX_FMT_LEFT) {
                tpx_memcpy(w, s.p, s.n);
                for (long long i = 0; i < pad; ++i) w[s.n + i] = ' ';
            } else {
                for (long long i = 0; i < pad; ++i) w[i] = ' ';
                tpx_memcpy(w + pad, s.p, s.n);
            }
            w += s.n + pad;
        }
    }
    return tstr{d, total};
}

// the ASCII whitespace of CPython's str.split(): wider than tpx_is_pyws by
// the separators FS GS RS US (0x1C-0x1F)
__device__ __forceinline__ bool tpx_is_splitws(unsigned char c) {
    return c == 0x20 || (c >= 0x09 && c <= 0x0d) || (c >= 0x1c && c <= 0x1f);
}

// string.capwords(s) == ' '.join(w.capitalize() for w in s.split())
TPX_FMT_FN tstr tpx_capwords(TpxHeap& h, const tstr s, int* ec) {
    long long words = 0, bytes = 0;
    bool in_word = false;
    for (long long i = 0; i < s.n; ++i) {
        const unsigned char c = (unsigned char)s.p[i];
        if (c >= 0x80) { *ec = EC_NCV; return tstr{s.p, 0}; }
        if (tpx_is_splitws(c)) {
            in_word = false;
        } else {
            if (!in_word) ++words;
            in_word = true;
            ++bytes;
        }
    }
    if (words == 0) return tstr{s.p, 0};
    const long long total = bytes + words - 1;
    char* d = tpx_alloc(h, total);
    if (!d) { *ec = EC_MEMORYERROR; return tstr{s.p, 0}; }
    char* w = d;
    in_word = false;
    for (long long i = 0; i < s.n; ++i) {
        const unsigned char c = (unsigned char)s.p[i];
        if (tpx_is_splitws(c)) {
            in_word = false;
        } else if (!in_word) {
            if (w != d) *w++ = ' ';
            *w++ = (c >= 'a' && c <= 'z') ? c - 32 : c;
            in_word = true;
        } else {
            *w++ = (c >= 'A' && c <= 'Z') ? c + 32 : c;
        }
    }
    return tstr{d, total};
}
