"""tests/native/deflate_tokens_main.cpp from Python: member texts and their tokens go in as files, the members the code builder
makes of them and the program's report come back.  The CPU tests build the program under the address and undefined-behaviour
sanitizers; the GPU tests, which only need its members, build it plain."""
import collections
import os
import shutil
import struct
import subprocess

from tests import helpers as H

CSRC = os.path.join(H.ROOT, "kreeq_amd", "csrc")
SOURCE = os.path.join(H.ROOT, "tests", "native", "deflate_tokens_main.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

Member = collections.namedtuple("Member", "data size dynamic max_lit_len max_dist_len max_token_bits")


def build(directory, sanitize):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(directory), "deflate_tokens")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + (SANITIZE if sanitize else []) + ["-I", CSRC, "-o", exe, SOURCE])
    return exe


def token_records(tokens):
    return b"".join(struct.pack("<HHB", 0, 0, t[0]) if len(t) == 1 else struct.pack("<HHB", t[0], t[1], 0) for t in tokens)


def make_members(exe, directory, items):
    """items: {name: (member text, tokens)} -> {name: Member}"""
    d = str(directory)
    os.makedirs(d, exist_ok=True)
    for name, (text, tokens) in items.items():
        with open(os.path.join(d, name + ".txt"), "wb") as f:
            f.write(text)
        with open(os.path.join(d, name + ".tok"), "wb") as f:
            f.write(token_records(tokens))
    p = subprocess.run([exe, d], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-4000:]
    lines = p.stdout.strip().split("\n")
    assert lines[-1] == "0 failures", lines[-1]
    out = {}
    for l in lines:
        if l.startswith("member "):
            f = l.split()
            with open(os.path.join(d, f[1] + ".gz"), "rb") as g:
                out[f[1]] = Member(g.read(), int(f[2]), bool(int(f[3])), int(f[4]), int(f[5]), int(f[6]))
    assert sorted(out) == sorted(items)
    return out


def restate(exe, directory, texts):
    """{name: text} -> {name: [(member text, restated tokens, Member) per member of the text]}: deflate_ref's parse through the
    code builder"""
    from tests import deflate_ref as R

    items = {}
    for name, text in texts.items():
        for i, piece in enumerate(R.members(text)):
            items["%s.%d" % (name, i)] = (piece, R.parse(piece))
    made = make_members(exe, directory, items)
    return {name: [items["%s.%d" % (name, i)] + (made["%s.%d" % (name, i)],) for i in range(len(R.members(text)))] for name, text in texts.items()}
