"""The ownership rule of the ABI layer, kept from eroding: kreeq_amd/csrc/kreeq_amd.hip takes and returns device memory,
pinned memory, events and streams only through the owners of kq_mem_host.h.  Outside comments, the runtime's allocation and
creation calls appear only inside `struct Scrambled` (its member functions are defined in its body).  String literals are
set aside with the comments: an error message may name a call (kq_create's "hipStreamCreate: ..." is part of the ABI's text)."""
import os
import re

from tests import helpers as H

SOURCE = os.path.join(H.ROOT, "kreeq_amd", "csrc", "kreeq_amd.hip")
CALLS = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree|hipEventCreate\w*|hipEventDestroy|hipStreamCreate\w*|hipStreamDestroy)\b")


def strip_comments(text):
    """the program text without its comments and without the content of string and character literals"""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if text.startswith("//", i):
            while i < n and text[i] != "\n":
                i += 1
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            j = n if j < 0 else j + 2
            out.append("".join(ch if ch == "\n" else " " for ch in text[i:j]))
            i = j
        elif c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(c + c)
            i = j + 1
        else:
            out.append(c)
            i += 1
    return "".join(out)


def struct_span(code, name):
    """[start, end) of `struct name { ... }`, by brace depth"""
    m = re.search(r"\bstruct\s+%s\s*\{" % name, code)
    assert m, "struct %s not found" % name
    depth, i = 0, m.end() - 1
    while True:
        depth += {"{": 1, "}": -1}.get(code[i], 0)
        i += 1
        if depth == 0:
            return m.start(), i


def test_strip_comments():
    assert strip_comments('a // hipFree(p)\nb /* hipMalloc\n */ c "// \\" hipFree" d \'"\' hipFree(e)').split() == ["a", "b", "c", '""', "d", "''", "hipFree(e)"]


def test_runtime_calls_only_in_scrambled():
    code = strip_comments(open(SOURCE).read())
    lo, hi = struct_span(code, "Scrambled")
    inside = [m.group(1) for m in CALLS.finditer(code) if lo <= m.start() < hi]
    outside = ["%s (line %d)" % (m.group(1), code.count("\n", 0, m.start()) + 1) for m in CALLS.finditer(code) if not lo <= m.start() < hi]
    assert not outside, "runtime allocation calls outside struct Scrambled: " + ", ".join(outside)
    assert "hipMalloc" in inside and "hipFree" in inside           # the search does find them where they are allowed
    # nothing outside the struct defines a member of it
    assert "Scrambled::" not in code
