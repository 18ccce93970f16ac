"""Constant regex pattern -> word program for the device VM (csrc/tpx_re.hip.h).

The pattern is parsed by CPython's own sre parser (re._parser on newer Pythons,
sre_parse before), so there is no second pattern grammar here: this module only
lowers the parse tree. Anything the parser yields that is not lowered on purpose
raises ReLowerError -> UDFCompileError -> the stage takes the interpreter path,
as every `re.` UDF did before. A pattern is never compiled approximately.

Character classes become 128-bit ASCII bitmaps; membership of every c < 128 is
asked of CPython itself (so `\\s` includes \\x1c-\\x1f for str patterns). Subject
bytes >= 0x80 that reach a class divert the row on the device.
"""
import re

try:  # Python >= 3.11
    import re._parser as _sre_parse
    import re._constants as _sre_c
except ImportError:  # pragma: no cover - depends on the interpreter
    import sre_parse as _sre_parse
    import sre_constants as _sre_c


class ReLowerError(Exception):
    pass


# opcodes / layout: keep in step with csrc/tpx_re.hip.h
H_SIZE = 4
OP_CHAR, OP_LIT, OP_CLASS, OP_SPAN, OP_SPLIT, OP_JMP, OP_SAVE, OP_SAVER, \
    OP_ASSERT, OP_MATCH = range(1, 11)
SPAN_LAZY, SPAN_NOBT = 1, 2
SPAN_INF = 0x7fffffff
AT_BOS, AT_EOL, AT_EOS, AT_WB, AT_NWB, AT_NWB_E = range(6)
# whether \B matches the empty string depends on the CPython version
_NWB_MATCHES_EMPTY = re.search(r"\B", "") is not None
MAX_WORDS = 2048
MAX_GROUPS = 31

_MAXREPEAT = _sre_c.MAXREPEAT

_CAT_PATTERNS = {
    "CATEGORY_DIGIT": r"\d", "CATEGORY_NOT_DIGIT": r"\D",
    "CATEGORY_SPACE": r"\s", "CATEGORY_NOT_SPACE": r"\S",
    "CATEGORY_WORD": r"\w", "CATEGORY_NOT_WORD": r"\W",
}
_CAT_CACHE = {}


def _category_set(cat):
    name = str(cat)
    if name not in _CAT_PATTERNS:
        raise ReLowerError("unsupported category %s" % name)
    if name not in _CAT_CACHE:
        rx = re.compile(_CAT_PATTERNS[name])
        _CAT_CACHE[name] = frozenset(
            c for c in range(128) if rx.fullmatch(chr(c)) is not None)
    return _CAT_CACHE[name]


def _ascii(c):
    if not (0 <= c < 128):
        raise ReLowerError("non-ASCII pattern character")
    return c


def _class_of(op, av):
    """ASCII member set of a one-character item, or None if `op` is not one."""
    name = str(op)
    if name == "LITERAL":
        return frozenset([_ascii(av)])
    if name == "NOT_LITERAL":
        return frozenset(range(128)) - {_ascii(av)}
    if name == "ANY":
        return frozenset(range(128)) - {10}  # no DOTALL: flags are rejected
    if name == "IN":
        neg = False
        members = set()
        for iop, iav in av:
            iname = str(iop)
            if iname == "NEGATE":
                neg = True
            elif iname == "LITERAL":
                members.add(_ascii(iav))
            elif iname == "RANGE":
                lo, hi = iav
                members.update(range(_ascii(lo), _ascii(hi) + 1))
            elif iname == "CATEGORY":
                members |= _category_set(iav)
            else:
                raise ReLowerError("unsupported set item %s" % iname)
        return frozenset(range(128)) - members if neg else frozenset(members)
    return None


def _bitmap(members):
    words = [0, 0, 0, 0]
    for c in members:
        words[c >> 5] |= 1 << (c & 31)
    return [w - (1 << 32) if w >= (1 << 31) else w for w in words]


def _min_width(items):
    total = 0
    for op, av in items:
        name = str(op)
        if name in ("LITERAL", "NOT_LITERAL", "ANY", "IN"):
            total += 1
        elif name == "SUBPATTERN":
            total += _min_width(av[3])
        elif name == "BRANCH":
            total += min(_min_width(b) for b in av[1])
        elif name in ("MAX_REPEAT", "MIN_REPEAT"):
            total += av[0] * _min_width(av[2])
        elif name == "AT":
            pass
        else:
            raise ReLowerError("unsupported construct %s" % name)
    return total


def _has_capture(items):
    for op, av in items:
        name = str(op)
        if name == "SUBPATTERN":
            if av[0] is not None or _has_capture(av[3]):
                return True
        elif name == "BRANCH":
            if any(_has_capture(b) for b in av[1]):
                return True
        elif name in ("MAX_REPEAT", "MIN_REPEAT"):
            if _has_capture(av[2]):
                return True
    return False


class _Lower:
    def __init__(self, ngroups):
        self.code = []
        self.ngroups = ngroups
        self.optional = set()   # groups seen where they may not take part
        self.mandatory = set()  # groups seen on every match path
        self.in_repeat = 0      # >0: a capture here can be overwritten

    def emit(self, *words):
        at = len(self.code)
        self.code.extend(words)
        if len(self.code) > MAX_WORDS:
            raise ReLowerError("pattern too large after repeat expansion")
        return at

    def seq(self, items, opt):
        run = []  # pending literal run

        def flush():
            if not run:
                return
            if len(run) == 1:
                self.emit(OP_CHAR, run[0])
            else:
                packed = []
                for i in range(0, len(run), 4):
                    w = 0
                    for j, c in enumerate(run[i:i + 4]):
                        w |= c << (8 * j)
                    packed.append(w - (1 << 32) if w >= (1 << 31) else w)
                self.emit(OP_LIT, len(run), *packed)
            del run[:]

        for op, av in items:
            name = str(op)
            if name == "LITERAL":
                run.append(_ascii(av))
                continue
            flush()
            self.item(name, op, av, opt)
        flush()

    def item(self, name, op, av, opt):
        if name in ("NOT_LITERAL", "ANY", "IN"):
            self.emit(OP_CLASS, *_bitmap(_class_of(op, av)))
        elif name == "AT":
            where = str(av)
            kind = {"AT_BEGINNING": AT_BOS, "AT_BEGINNING_STRING": AT_BOS,
                    "AT_END": AT_EOL, "AT_END_STRING": AT_EOS,
                    "AT_BOUNDARY": AT_WB, "AT_NON_BOUNDARY": AT_NWB}.get(where)
            if kind is None:
                raise ReLowerError("unsupported anchor %s" % where)
            if kind == AT_NWB and _NWB_MATCHES_EMPTY:
                kind = AT_NWB_E
            bm = _bitmap(_category_set("CATEGORY_WORD")) \
                if kind in (AT_WB, AT_NWB, AT_NWB_E) else [0, 0, 0, 0]
            self.emit(OP_ASSERT, kind, *bm)
        elif name == "SUBPATTERN":
            group, add_flags, del_flags, sub = av
            if add_flags or del_flags:
                raise ReLowerError("inline flags are not supported")
            if group is None:
                self.seq(sub, opt)
                return
            (self.optional if opt else self.mandatory).add(group)
            save = OP_SAVER if (opt or self.in_repeat) else OP_SAVE
            self.emit(save, 2 * group)
            self.seq(sub, opt)
            self.emit(save, 2 * group + 1)
        elif name == "BRANCH":
            _, alts = av
            # SPLIT a1, next; a1; JMP end; next: SPLIT a2, ...; last; end:
            jumps = []
            for i, alt in enumerate(alts):
                last = i == len(alts) - 1
                if not last:
                    sp = self.emit(OP_SPLIT, 0, 0)
                    self.code[sp + 1] = len(self.code)
                self.seq(alt, True)
                if not last:
                    jumps.append(self.emit(OP_JMP, 0))
                    self.code[sp + 2] = len(self.code)
            for j in jumps:
                self.code[j + 1] = len(self.code)
        elif name in ("MAX_REPEAT", "MIN_REPEAT"):
            self.repeat(name == "MIN_REPEAT", av, opt)
        else:
            # GROUPREF, GROUPREF_EXISTS, ASSERT, ASSERT_NOT, ATOMIC_GROUP,
            # POSSESSIVE_REPEAT, ...
            raise ReLowerError("unsupported construct %s" % name)

    def repeat(self, lazy, av, opt):
        mn, mx, body = av
        body = list(body)
        inf = mx == _MAXREPEAT
        if not inf and mx < mn:
            raise ReLowerError("bad repeat bounds")
        single = _class_of(*body[0]) if len(body) == 1 else None
        if single is not None:
            if mn >= SPAN_INF or (not inf and mx >= SPAN_INF):
                raise ReLowerError("repeat bound too large")
            self.emit(OP_SPAN, mn, SPAN_INF if inf else mx,
                      SPAN_LAZY if lazy else 0, *_bitmap(single))
            return
        if _min_width(body) == 0:
            raise ReLowerError("repeated group whose body can match the "
                               "empty string")
        if lazy and (inf or mx > 1) and _has_capture(body):
            # CPython before 3.11 does not restore a capture when it
            # backtracks out of an iteration of a lazy group repeat (spans
            # with start > end come out): version-dependent, so not compiled
            raise ReLowerError("capture group inside a lazy group repeat")
        self.in_repeat += 1
        try:
            self._repeat_body(lazy, mn, mx, inf, body, opt)
        finally:
            self.in_repeat -= 1

    def _repeat_body(self, lazy, mn, mx, inf, body, opt):
        for _ in range(mn):
            self.seq(body, opt)
        inner_opt = True
        if inf:
            top = self.emit(OP_SPLIT, 0, 0)
            self.code[top + 1] = len(self.code)
            self.seq(body, inner_opt)
            self.emit(OP_JMP, top)
            out = len(self.code)
            self.code[top + 2] = out
            if lazy:
                self.code[top + 1], self.code[top + 2] = out, top + 3
            return
        splits = []
        for _ in range(mx - mn):
            sp = self.emit(OP_SPLIT, 0, 0)
            self.code[sp + 1] = len(self.code)
            splits.append(sp)
            self.seq(body, inner_opt)
        out = len(self.code)
        for sp in splits:
            if lazy:
                self.code[sp + 2] = self.code[sp + 1]
                self.code[sp + 1] = out
            else:
                self.code[sp + 2] = out


def _first_real(code, pc):
    """pc of the first instruction at/after pc that is not a capture save."""
    while code[pc] in (OP_SAVE, OP_SAVER):
        pc += 2
    return pc


def _instr_len(code, pc):
    op = code[pc]
    if op == OP_LIT:
        return 2 + (code[pc + 1] + 3) // 4
    return {OP_CHAR: 2, OP_CLASS: 5, OP_SPAN: 8, OP_SPLIT: 3, OP_JMP: 2,
            OP_SAVE: 2, OP_SAVER: 2, OP_ASSERT: 6, OP_MATCH: 1}[op]


def _first_byte(code, pc):
    op = code[pc]
    if op == OP_CHAR:
        return code[pc + 1]
    if op == OP_LIT:
        return code[pc + 2] & 255
    return None


def _mark_nobt(code):
    """A greedy span directly followed by a literal byte outside its class can
    never succeed after shrinking (the byte at the shrunk end is in the class):
    mark it so the VM pushes no backtrack frame."""
    pc = 0
    while pc < len(code):
        if code[pc] == OP_SPAN and not (code[pc + 3] & SPAN_LAZY):
            nxt = _first_real(code, pc + 8)
            b = _first_byte(code, nxt)
            if b is not None:
                word = code[pc + 4 + (b >> 5)] & 0xffffffff
                if not (word >> (b & 31)) & 1:
                    code[pc + 3] |= SPAN_NOBT
        pc += _instr_len(code, pc)


class Program:
    """words: the VM program; ngroups; optional: group numbers that can be
    None after a successful match."""

    def __init__(self, words, ngroups, optional):
        self.words = words
        self.ngroups = ngroups
        self.optional = frozenset(optional)


_PROGRAM_CACHE = {}


def lower(pattern, mode="search"):
    """mode: search | match | fullmatch."""
    key = (pattern, mode)
    if key not in _PROGRAM_CACHE:
        _PROGRAM_CACHE[key] = _lower(pattern, mode)
    return _PROGRAM_CACHE[key]


def _lower(pattern, mode):
    if not isinstance(pattern, str):
        raise ReLowerError("pattern must be a str")
    if mode not in ("search", "match", "fullmatch"):
        raise ReLowerError("unsupported re function %s" % mode)
    try:
        tree = _sre_parse.parse(pattern, 0)
    except (re.error, RecursionError, OverflowError) as e:
        raise ReLowerError("bad pattern: %s" % e)
    state = getattr(tree, "state", None) or getattr(tree, "pattern")
    if state.flags & ~_sre_c.SRE_FLAG_UNICODE:
        raise ReLowerError("inline flags are not supported")
    ngroups = state.groups - 1
    if ngroups > MAX_GROUPS:
        raise ReLowerError("too many groups")
    lw = _Lower(ngroups)
    lw.seq(list(tree), False)
    if mode == "fullmatch":
        lw.emit(OP_ASSERT, AT_EOS, 0, 0, 0, 0)
    lw.emit(OP_MATCH)
    code = lw.code
    _mark_nobt(code)
    start = _first_real(code, 0)
    anchored = mode != "search" or (
        code[start] == OP_ASSERT and code[start + 1] == AT_BOS)
    first = None if anchored else _first_byte(code, start)
    # rebase jump targets past the header
    pc = 0
    while pc < len(code):
        if code[pc] == OP_SPLIT:
            code[pc + 1] += H_SIZE
            code[pc + 2] += H_SIZE
        elif code[pc] == OP_JMP:
            code[pc + 1] += H_SIZE
        pc += _instr_len(code, pc)
    header = [2 * (ngroups + 1), 1 if anchored else 0,
              -1 if first is None else first, H_SIZE + len(code)]
    return Program(header + code, ngroups, lw.optional - lw.mandatory)
