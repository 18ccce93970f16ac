"""Key vectors for the device join table tests (host: test_host_join.py,
GPU: test_gpu_join_table.py), built with the host hash model of
codegen.StageCodegen (_jhash_i64 / _jhash_bytes — the replica of the device
hashes the embedded table is built with)."""
import random

import numpy as np

from tuplex_amd.codegen import StageCodegen

SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000]
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
# tests/hipkern.py's poison value: what an untouched output buffer reads as
POISON_I64 = int(np.frombuffer(bytes([0xA5]) * 8, dtype=np.int64)[0])
N_COLLIDE = 12

hash_i64 = StageCodegen._jhash_i64
hash_bytes = StageCodegen._jhash_bytes


def table_size(n):
    """Smallest power of two >= 2 n, at least 8 (the embedded table's rule)."""
    tsize = 8
    while tsize < 2 * max(n, 1):
        tsize <<= 1
    return tsize


_wrap_i64_cache = {}


def wrap_i64(tsize, count):
    """`count` int64 keys whose home slot is tsize - 1: probing wraps."""
    have = _wrap_i64_cache.setdefault(tsize, [])
    k = (have[-1] + 1) if have else 1000003
    while len(have) < count:
        if hash_i64(k) & (tsize - 1) == tsize - 1:
            have.append(k)
        k += 1
    return have[:count]


_wrap_str_cache = {}


def wrap_str(tsize, count):
    """`count` strings "c<i>" whose home slot is tsize - 1."""
    have = _wrap_str_cache.setdefault(tsize, [])
    i = (int(have[-1][1:]) + 1) if have else 0
    while len(have) < count:
        s = "c%d" % i
        if hash_bytes(s.encode()) & (tsize - 1) == tsize - 1:
            have.append(s)
        i += 1
    return have[:count]


def i64_case(n):
    """(build keys [n], absent keys) for a build side of n rows."""
    tsize = table_size(n)
    special = [0, -1, INT64_MIN, INT64_MAX, POISON_I64]
    wrap = wrap_i64(tsize, N_COLLIDE + 4)
    if n <= 2:
        keys = [[], [-1], [0, POISON_I64]][n]
    else:
        keys = (special + wrap[:N_COLLIDE])[:n]
    rng = random.Random(4100 + n)
    have = set(keys)
    while len(keys) < n:
        k = rng.randrange(INT64_MIN, INT64_MAX + 1)
        if k not in have:
            have.add(k)
            keys.append(k)
    absent = [k for k in special + [1, -2, INT64_MIN + 1, INT64_MAX - 1,
                                    POISON_I64 + 1] + wrap
              if k not in have]
    absent += [k + 1 for k in keys[:8] if k + 1 not in have
               and k + 1 <= INT64_MAX]
    rng.shuffle(keys)
    return keys, absent


def str_case(n):
    """(build keys [n], absent keys), python strings."""
    tsize = table_size(n)
    special = ["", "a", "b", "ab", "abc", "abd", "x" * 299 + "y",
               "é", "日本", "日本語", "\U0001f642"]
    wrap = wrap_str(tsize, N_COLLIDE + 4)
    if n <= 2:
        keys = [[], [""], ["ab", "abc"]][n]
    else:
        keys = (special + wrap[:N_COLLIDE])[:n]
    have = set(keys)
    i = 0
    while len(keys) < n:
        s = "k%05d" % i
        i += 1
        if s not in have:
            have.add(s)
            keys.append(s)
    absent = [s for s in special + ["abx", "ab\x00", "A", "x" * 300,
                                    "x" * 299 + "z", "x" * 298 + "y",
                                    "日", "è", "k99999", "c"] + wrap
              if s not in have]
    random.Random(4200 + n).shuffle(keys)
    return keys, absent
