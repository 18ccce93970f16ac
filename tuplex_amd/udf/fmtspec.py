"""Constant format templates -> field descriptors for the device string builder.

`S.format(a0, ..)` and `S % (a0, ..)` with a compile-time S are parsed here into
a flat item list; udf/compile.py hangs it on one TIR `format` node, codegen.py
embeds `encode(items)` next to the stage's literals, and tpx_format()
(csrc/tpx_fmt.hip.h) walks it twice: once for the exact length, once to write.

items:
  ("lit", text)
  ("int", arg, flags, width)   i64 (or bool printed as 1/0); right-aligned
                               unless FLAG_LEFT; FLAG_ZERO pads sign-aware
  ("str", arg, flags, width)   str; right-aligned unless FLAG_LEFT
  ("bool", arg)                bool printed as True/False, no width

Argument kinds ('i' i64, 'b' bool, 's' str) are static, so every directive that
CPython would reject at run time for that kind is rejected here.
"""
import re
import string

FLAG_ZERO = 1
FLAG_LEFT = 2
MAX_WIDTH = 255
MAX_ARGS = 32


class FmtError(Exception):
    pass


def _width(text):
    w = int(text) if text else 0
    if w > MAX_WIDTH:
        raise FmtError("format width %d above %d" % (w, MAX_WIDTH))
    return w


def _push_lit(items, text):
    if not text:
        return
    if items and items[-1][0] == "lit":
        items[-1] = ("lit", items[-1][1] + text)
    else:
        items.append(("lit", text))


def _check_args(used, kinds, strict):
    if len(kinds) > MAX_ARGS:
        raise FmtError("more than %d format arguments" % MAX_ARGS)
    if strict and used != set(range(len(kinds))):
        raise FmtError("format arguments and fields do not pair up")


_FORMAT_INT = re.compile(r"(0?)(\d*)(d?)\Z")
# a width that starts with 0 is CPython's zero-fill flag ('{:05}' on 'ab' is
# 'ab000'): not in the subset, so a str width has no leading zero
_FORMAT_STR = re.compile(r"([<>]?)([1-9]\d*)?(s?)\Z")


def parse_format(template, kinds):
    """str.format subset: {} / {k}, {{ }} escapes, int spec [0][width][d],
    str spec [<|>][width][s], bool only with an empty spec."""
    items = []
    auto = None
    nxt = 0
    used = set()
    try:
        parts = list(string.Formatter().parse(template))
    except ValueError as e:
        raise FmtError("format template: %s" % e)
    for lit, field, spec, conv in parts:
        _push_lit(items, lit)
        if field is None:
            continue
        if conv is not None:
            raise FmtError("format conversion !%s is not supported" % conv)
        if field == "":
            if auto is False:
                raise FmtError("cannot switch from manual field specification "
                               "to automatic field numbering")
            auto = True
            k = nxt
            nxt += 1
        elif field.isdigit():
            if auto is True:
                raise FmtError("cannot switch from automatic field numbering "
                               "to manual field specification")
            auto = False
            k = int(field)
        else:
            raise FmtError("format field %r (only {} and {k})" % field)
        if k >= len(kinds):
            raise FmtError("format field %d has no argument" % k)
        used.add(k)
        kind = kinds[k]
        if kind == "b":
            if spec:
                raise FmtError("bool formats only with an empty spec")
            items.append(("bool", k))
        elif kind == "i":
            m = _FORMAT_INT.match(spec)
            if not m:
                raise FmtError("unsupported int format spec %r" % spec)
            items.append(("int", k, FLAG_ZERO if m.group(1) else 0,
                          _width(m.group(2))))
        elif kind == "s":
            m = _FORMAT_STR.match(spec)
            if not m:
                raise FmtError("unsupported str format spec %r" % spec)
            items.append(("str", k, 0 if m.group(1) == ">" else FLAG_LEFT,
                          _width(m.group(2))))
        else:
            raise FmtError("format argument kind %r" % kind)
    # CPython ignores surplus positional arguments; a template that names
    # fewer than it is given is more likely a slip, and stays uncompiled
    _check_args(used, kinds, strict=True)
    return items


_PERCENT = re.compile(r"%(?:(%)|([-0]?)([1-9]\d*)?([ds]))")


def parse_percent(template, kinds):
    """printf-style subset: %d %0Nd %Nd %s %Ns %-Ns %%."""
    items = []
    pos = 0
    k = 0
    while True:
        i = template.find("%", pos)
        if i < 0:
            _push_lit(items, template[pos:])
            break
        _push_lit(items, template[pos:i])
        m = _PERCENT.match(template, i)
        if not m:
            raise FmtError("unsupported format spec %r" % template)
        pos = m.end()
        if m.group(1):
            _push_lit(items, "%")
            continue
        flag, width, conv = m.group(2), _width(m.group(3)), m.group(4)
        if k >= len(kinds):
            raise FmtError("not enough arguments for format string")
        kind = kinds[k]
        if conv == "d":
            if flag == "-":
                raise FmtError("unsupported format spec %r" % template)
            if kind == "s":
                raise FmtError("%d format needs a number")
            items.append(("int", k, FLAG_ZERO if flag == "0" else 0, width))
        else:
            if flag == "0":
                raise FmtError("unsupported format spec %r" % template)
            left = FLAG_LEFT if flag == "-" else 0
            if kind == "i":
                items.append(("int", k, left, width))
            elif kind == "s":
                items.append(("str", k, left, width))
            elif width:
                raise FmtError("bool formats with %s only without a width")
            else:
                items.append(("bool", k))
        k += 1
    if k != len(kinds):
        raise FmtError("not all arguments converted during string formatting")
    _check_args(set(range(k)), kinds, strict=False)
    return items


def encode(items):
    """(words, blob): four ints per item for tpx_format() —
    [0, offset, length, 0] for a literal (bytes blob[offset:offset+length]),
    [1, arg, flags, width] for an int, [2, arg, flags, width] for a str (a
    `bool` item is a str field: the caller passes its True/False text)."""
    words = []
    blob = b""
    for it in items:
        if it[0] == "lit":
            b = it[1].encode("utf-8")
            words += [0, len(blob), len(b), 0]
            blob += b
        elif it[0] == "int":
            words += [1, it[1], it[2], it[3]]
        elif it[0] == "str":
            words += [2, it[1], it[2], it[3]]
        else:
            words += [2, it[1], FLAG_LEFT, 0]
    return words, blob
