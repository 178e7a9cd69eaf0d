"""Inputs for the LZ77 parse of k_bgzf_deflate, one edge each, and for every input a predicate on the RESTATED tokens
(tests/deflate_ref.py) that proves the edge is present: tests/test_deflate_ref.py evaluates the predicates on the CPU, so that
the comparison of the device with the restatement (tests/test_gpu_deflate_parse.py) cannot pass on inputs that miss their edge.

A case is (name, text, check).  check(at, made) raises AssertionError when the edge is absent; `at` holds, per member of the
text, the list [(text position in the member, token)] of deflate_ref.parse_at, `made` the members the code builder made of these
tokens (deflate_native.Member, per member of the text), or None where only the tokens are at hand (the seed search).

The parse sees a candidate only through a 12-bit hash slot that any later trigram may take, so random stretches are drawn
from a seed and the seed is searched until the predicate holds (`python -m tests.deflate_cases` prints the seeds; SEEDS
records them, so that importing this module searches nothing).  Stretches that must stay quiet are runs of one byte value
below 16: a run costs one slot.  Random stretches use the values 16..255."""
import bisect
import collections
import heapq

import numpy as np

from tests import bgzf_inputs as B
from tests import deflate_ref as R

MEMBER = R.MEMBER
Case = collections.namedtuple("Case", "name text check")

QUICK_LENGTHS = (3, 4, 5, 31, 32, 33, 35, 36, 37, 257, 258, 259, 300)
END_LEFT = (1, 2, 3, 4, 31, 32, 33, 258)
END_N = (1000, 63, 64, 65, 127, 128, 129, 64 * 1020 - 1, 64 * 1020, 64 * 1020 + 1)
KIND_ALPHABETS, KIND_LENGTHS = (256, 250, 200), (20, 60, 200, 1000)

# the seed each searched case settled on (the first at which its predicate holds), where that is not 0
SEEDS = {'quick_31': 1, 'quick_257': 1, 'end_n129_left3': 1, 'end_n129_left4': 2, 'end_n65280_left3': 1, 'end_n65280_left4': 1,
         'end_n65280_left31': 1, 'end_n65281_left32': 1, 'step_geometry': 1}


def rand(rng, n, lo=16, hi=256):
    return rng.integers(lo, hi, n).astype(np.uint8).tobytes()


def other_than(b):
    """a byte of the random range that is not b"""
    return bytes([16 + (b - 16 + 97) % 240])


def run(value, n):
    return bytes([value]) * n


# A member is coded only where that is shorter than storing it, and a stored member shows no token: short random texts end with
# this run, which a few matches cover.  must_be_coded() is asked of every member by the CPU test.
CHEAP_TAIL = run(12, 1500)


def must_be_coded(name, n_text):
    """whether a member of n_text bytes of the case has to come out as a dynamic block for the case to test anything"""
    return not name.startswith("kind_") and n_text >= 20


def is_literals(tokens, text):
    return [t for _, t in tokens] == [(b,) for b in text]


def same_step(p, dist):
    return (p - dist) // R.STEP == p // R.STEP


# ---- the quick length of 32 and the cap of 258 ---------------------------------------------------------------------------------
def quick_length(L, seed):
    rng = np.random.default_rng([1, L, seed])
    src = rand(rng, 400)
    text = src + run(0, 100) + src[:L] + other_than(src[L]) + run(1, 70)
    p0 = 500

    def check(at, made):
        d = dict(at[0])
        assert d.get(p0) == (min(L, 258), p0), d.get(p0)
        if L > 258:                                                 # the cap leaves a rest: another token follows
            assert p0 + 258 in d
        if L == 300:
            assert d[p0 + 258] == (42, p0)
    return text, check


# ---- a copy that runs into the end of the member ---------------------------------------------------------------------------------
def end_shape(n, left):
    """(lead, length of the source, gap) of a text of n bytes whose last `left` bytes repeat what begins with the source, or None.
    Where the source and the gap are shorter than `left`, the repeat overlaps its own source, as a DEFLATE match may."""
    gap = 3 if n < 200 else 70
    src = min(300, n - left - gap)
    return (n - left - gap - src, src, gap) if src >= 3 else None


def end_of_text(n, left, seed):
    full = min(n, MEMBER)                                           # n = 0xff01: the full member, and a member of one byte
    lead, ns, gap = end_shape(full, left)
    rng = np.random.default_rng([2, n, left, seed])
    src = rand(rng, ns) if n >= 200 else rand(rng, ns, 16, 22)     # (six letters: so short a text is stored unless it is cheap to code)
    copy = ((src + run(1, gap)) * (left // (ns + gap) + 1))[:left]
    text = run(0, lead) + src + run(1, gap) + copy + run(7, n - full)
    assert len(text) == n

    def check(at, made):
        p = full - left
        if left < R.MIN_MATCH:                                      # too short for a match: literals
            assert at[0][-left:] == [(p + i, (copy[i],)) for i in range(left)], at[0][-3:]
        else:                                                       # the match, clipped at the end of the text
            assert at[0][-1] == (p, (min(left, 258), ns + gap)), at[0][-3:]
        assert len(at) == (2 if n > MEMBER else 1)
        if n > MEMBER:
            assert at[1] == [(0, (7,))]
    return text, check


# ---- where matches start and end within the steps ------------------------------------------------------------------------------
GEOMETRY = ((0, 10), (63, 10), (20, 44), (20, 45), (60, 137))      # (lane of the start, length): lane 0, lane 63, ending on the last
#                                                                     position of a step, on the first of the next, over two whole steps


def step_geometry(seed):
    rng = np.random.default_rng([3, seed])
    src = rand(rng, 400)
    text, placed = src, []
    for i, (lane, L) in enumerate(GEOMETRY):
        text += run(i, (lane - len(text)) % 64 + 64)
        off = 50 * i
        placed.append((len(text), L, off))
        text += src[off:off + L] + other_than(src[off + L])
    text += run(9, 40)

    def check(at, made):
        d = dict(at[0])
        for p, L, off in placed:
            assert p % 64 == GEOMETRY[placed.index((p, L, off))][0]
            assert d.get(p) == (L, p - off), (p, d.get(p))
        p, L, _ = placed[2]
        assert (p + L - 1) % 64 == 63 and p + L in d                # ends on the last position of a step
        p, L, _ = placed[3]
        assert (p + L - 1) % 64 == 0 and p + L in d                 # on the first of the next
        p, L, _ = placed[4]
        base = (p // 64 + 1) * 64                                   # two whole steps inside the match produce no token
        assert p + L >= base + 128 and not any(base <= q < base + 128 for q in d)
        assert min(q for q in d if q > p) == p + L                  # and the next token starts where `covered` says
    return text, check


# ---- the window of 32 768 --------------------------------------------------------------------------------------------------------
def window(dist, lead, seed):
    rng = np.random.default_rng([4, lead, seed])                    # (the same stretch at both distances)
    x = rand(rng, 40)
    text = run(3, lead) + x + run(0, dist - 40) + x + run(1, 30)
    p0 = lead + dist

    def check(at, made):
        d = dict(at[0])
        hs = R.hashes(text)
        quiet = {hs[lead + dist - 3], hs[lead + dist - 2], hs[lead + dist - 1], hs[lead + 38], hs[lead + 39]}      # the zero and boundary trigrams
        assert not quiet & set(hs[lead:lead + 38])
        assert p0 in d
        if dist <= R.WINDOW:
            assert d[p0] == (40, dist), d[p0]
        else:
            inside = [(q, t) for q, t in at[0] if p0 <= q < p0 + 40]
            assert all(len(t) == 1 or (t[0] < 40 and t[1] < dist) for _, t in inside)
            assert is_literals(inside, x)                           # (a random stretch has no nearer match to offer)
            assert all(len(t) == 1 or t[1] <= R.WINDOW for _, t in at[0])
    return text, check


# ---- 3-byte matches further back than 4096 ---------------------------------------------------------------------------------------
def too_far(seed):
    rng = np.random.default_rng([5, seed])
    t1, t2, q4 = rand(rng, 3), rand(rng, 3), rand(rng, 4)
    buf = bytearray(13000)
    spots = ((100, t1, 4096), (4300, t2, 4097), (8500, q4, 4097))
    for a, word, dist in spots:
        buf[a:a + len(word)] = word                                 # between zeros
        b = a + dist
        buf[b - 1:b + len(word) + 1] = bytes([13]) + word + bytes([14])      # the repeat neither starts earlier nor goes on
    text = bytes(buf)

    def check(at, made):
        d = dict(at[0])
        assert d.get(100 + 4096) == (3, 4096)
        assert d.get(4300 + 4097) == (t2[0],) and not any(t == (3, 4097) for _, t in at[0])
        assert d.get(8500 + 4097) == (4, 4097)
    return text, check


# ---- matches whose source lies in the step of their start ------------------------------------------------------------------------
def in_step(kind, seed):
    rng = np.random.default_rng([6, seed])
    tail = rand(rng, 20) + CHEAP_TAIL
    if kind == "run":                                               # a run that starts in lane 20
        text = rand(rng, 84) + run(5, 30) + tail
        want = {84: (5,), 85: (29, 1)}
    elif kind == "period2":
        text = rand(rng, 74) + bytes([5, 6]) * 15 + tail
        want = {74: (5,), 75: (6,), 76: (28, 2)}
    elif kind == "period3":
        text = rand(rng, 74) + bytes([5, 6, 7]) * 10 + tail
        want = {74: (5,), 75: (6,), 76: (7,), 77: (27, 3)}
    elif kind == "interleaved":                                     # two repeats with different hashes, interleaved in one step
        a, b = rand(rng, 9), rand(rng, 9)
        text = rand(rng, 70) + a + run(1, 1) + b + run(2, 1) + a + run(3, 1) + b + run(4, 1) + tail
        assert R.hashes(a)[0] != R.hashes(b)[0]
        want = {90: (9, 20), 100: (9, 20)}
    elif kind == "letter64":                                        # one letter over exactly one step
        text = rand(rng, 64) + run(5, 64) + tail
        want = {64: (5,), 65: (63, 1)}
    else:                                                           # "lowest": three occurrences in a step; the third takes the first
        t = rand(rng, 3)
        buf = bytearray(rand(rng, 64 + 64))
        for i, p in enumerate((69, 84, 104)):                      # (its neighbours differ each time: 3 bytes and no more)
            buf[p - 1:p + 4] = bytes([1 + i]) + t + bytes([9 + i])
        text = bytes(buf) + tail
        want = {84: (3, 15), 104: (3, 35)}

    def check(at, made):
        d = dict(at[0])
        for p, t in want.items():
            assert d.get(p) == t, (p, d.get(p))
            assert len(t) == 1 or same_step(p, t[1])
    return text, check


# ---- the highest position of a step wins its slot ---------------------------------------------------------------------------------
def insert_order(seed):
    rng = np.random.default_rng([7, seed])
    t = rand(rng, 3)
    buf = bytearray(rand(rng, 300))
    for i, p in enumerate((69, 94, 202)):                           # twice in the step 64..127, again two steps later
        buf[p - 1:p + 4] = bytes([1 + i]) + t + bytes([9 + i])
    text = bytes(buf) + CHEAP_TAIL

    def check(at, made):
        assert dict(at[0]).get(202) == (3, 202 - 94)                # the later match points at the second occurrence
    return text, check


# ---- two trigrams in one slot -----------------------------------------------------------------------------------------------------
def hash_collision(seed):
    rng = np.random.default_rng([8, seed])
    pool = rand(rng, 3 * 3000)
    by_hash = {}
    u = v = None
    for i in range(0, len(pool), 3):
        t = pool[i:i + 3]
        o = by_hash.setdefault(R.hashes(t)[0], t)
        if o != t:
            u, v = o, t
            break
    assert u is not None
    buf = bytearray(rand(rng, 400))
    for i, (p, t) in enumerate(((70, u), (140, v), (260, u), (290, u))):      # u, then v in its slot, then u twice in the step 256..319
        buf[p - 1:p + 4] = bytes([1 + i]) + t + bytes([9 + i])
    text = bytes(buf) + CHEAP_TAIL

    def check(at, made):
        d = dict(at[0])
        hs = R.hashes(text)
        assert u != v and hs[70] == hs[140] == hs[260] == hs[290]
        assert max(p for p in range(256) if hs[p] == hs[260]) == 140      # the candidate both see is v's position
        assert d.get(260) == (u[0],)                                # no match there and nothing lower in the step: a literal
        assert d.get(290) == (3, 30)                                # the fallback inside the step
    return text, check


# ---- code lengths at the 15-bit limit ---------------------------------------------------------------------------------------------
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)


def unlimited_depths(tokens):
    """how deep Huffman codes WITHOUT a length limit would be for these tokens: (literal / length set, distance set)"""
    lit, dist = collections.Counter({256: 1}), collections.Counter()
    for t in tokens:
        if len(t) == 1:
            lit[t[0]] += 1
        else:
            lit[257 + bisect.bisect_right(LEN_BASE, t[0]) - 1] += 1
            dist[bisect.bisect_right(DIST_BASE, t[1]) - 1] += 1

    def depth(counts):
        heap = [(c, i, 0) for i, c in enumerate(counts.values())]
        heapq.heapify(heap)
        k = len(heap)
        while len(heap) > 1:
            x, y = heapq.heappop(heap), heapq.heappop(heap)
            k += 1
            heapq.heappush(heap, (x[0] + y[0], k, max(x[2], y[2]) + 1))
        return heap[0][2] if heap else 0
    return depth(lit), depth(dist)


def skewed_literals(seed):
    """Byte counts 1, 2, 3, 5, 8 .. 987 (15 Fibonacci numbers) on the values 0..14, and 64 more values about 980 times each,
    shuffled: 79 symbols in a full member.  The rare values form a chain 15 deep that hangs below the 6 levels of the frequent
    ones.  (A member has no room for 30 Fibonacci counts, and with fewer, more frequent values the parse finds matches whose
    length codes break the chain; the predicate, not the recipe, says what the case must reach.)"""
    rng = np.random.default_rng([9, seed])
    f = [1, 2]
    while len(f) < 15:
        f.append(f[-1] + f[-2])
    rare = np.repeat(np.arange(15, dtype=np.uint8), f)
    data = np.concatenate([rare, rng.integers(192, 256, MEMBER - len(rare)).astype(np.uint8)])
    rng.shuffle(data)

    def check(at, made):
        tokens = [t for _, t in at[0]]
        assert len({t[0] for t in tokens if len(t) == 1}) >= 30
        assert unlimited_depths(tokens)[0] > 15                     # the limit is needed, not just met
        if made is not None:
            assert made[0].dynamic and made[0].max_lit_len == 15, made[0][1:]
            assert made[0].max_token_bits <= 48
    return data.tobytes(), check


# distance symbol -> how many matches of it the text asks for: Fibonacci counts on the near symbols, where the parse finds every
# copy, then a steeper sequence, since a far copy is lost when another trigram takes its slot
SKEWED_DISTANCES = ((4, 1), (5, 1), (6, 2), (7, 3), (8, 5), (9, 8), (10, 13), (11, 22), (12, 36), (0, 59), (1, 97), (13, 160), (14, 264),
                    (15, 440), (16, 780), (3, 1190), (2, 1960))


def skewed_distances(seed):
    """Matches of 3 bytes at chosen distances: a few fresh random bytes, then 3 bytes copied from `d` back, then a byte that
    ends the match.  Every source is fresh (never copied, and no copy itself), and no trigram besides the copied one occurs
    twice, so the parse has no other match to find: 17 distance symbols whose counts form a chain 16 deep."""
    rng = np.random.default_rng([10, seed])
    symbols = np.repeat(np.array([s for s, _ in SKEWED_DISTANCES]), [c for _, c in SKEWED_DISTANCES])
    rng.shuffle(symbols)
    buf, fresh, seen = bytearray(), bytearray(), set()

    def new_byte(avoid=None):
        while True:
            b = int(rng.integers(16, 256))
            if b != avoid and bytes(buf[-2:]) + bytes([b]) not in seen:
                return b

    def push(b, is_fresh):
        buf.append(b)
        fresh.append(is_fresh)
        if len(buf) >= 3:
            seen.add(bytes(buf[-3:]))

    for _ in range(64):
        push(new_byte(), 1)
    for s in symbols.tolist():
        for _ in range(int(rng.integers(2, 4))):
            push(new_byte(), 1)
        while True:                                                 # a distance of the symbol whose source is fresh; else one more fresh byte
            p = len(buf)
            lo, hi = DIST_BASE[s], DIST_BASE[s + 1]
            ok = []
            for d in (range(lo, hi) if hi - lo <= 32 else rng.integers(lo, hi, 32).tolist()):
                if d > p or not all(fresh[p - d:min(p, p - d + 3)]):
                    continue
                w = bytearray()
                for j in range(3):
                    w.append((buf + w)[p + j - d])
                t = bytes(buf[-2:] + w)
                if t[0:3] not in seen and t[1:4] not in seen:       # the two trigrams that run into the copy are new
                    ok.append((d, w))
            if ok:
                break
            push(new_byte(), 1)
        d, w = ok[int(rng.integers(len(ok)))]
        for i in range(p - d, min(p, p - d + 3)):
            fresh[i] = 0
        for b in w:
            push(b, 0)
        push(new_byte(avoid=buf[len(buf) - d]), 1)
    assert len(buf) <= MEMBER
    text = bytes(buf)

    def check(at, made):
        tokens = [t for _, t in at[0]]
        assert unlimited_depths(tokens)[1] > 15
        if made is not None:
            assert made[0].dynamic and made[0].max_dist_len == 15, made[0][1:]
            assert made[0].max_token_bits <= 48
    return text, check


# ---- dynamic or stored ------------------------------------------------------------------------------------------------------------
def kind(alphabet, n):
    rng = np.random.default_rng([11, alphabet, n])
    return rand(rng, n, 0, alphabet), lambda at, made: None         # (the test asks that both kinds occur among KIND_NAMES)


KIND_NAMES = ["kind_a%d_n%d" % (a, n) for a in KIND_ALPHABETS for n in KIND_LENGTHS]


# ---- no window crosses a member ---------------------------------------------------------------------------------------------------
def member_boundary(seed):
    rng = np.random.default_rng([12, seed])
    src = rand(rng, 300)
    text = run(0, MEMBER - 300) + src + src + run(1, MEMBER - 300) + src[:20] + run(2, 80)
    assert len(text) == 2 * MEMBER + 100

    def check(at, made):
        assert len(at) == 3
        assert is_literals(at[1][:100], src[:100])                  # the second member starts with what the first ended with: literals
        assert is_literals(at[2][:20], src[:20])
        assert at[0][-1][1] == (src[-1],)
    return text, check


def realistic():
    return B.fastq_text(3 * MEMBER, seed=5), lambda at, made: None


def builders():
    """{name: builder(seed) -> (text, check)}"""
    out = collections.OrderedDict()
    for L in QUICK_LENGTHS:
        out["quick_%d" % L] = lambda seed, L=L: quick_length(L, seed)
    for n in END_N:
        for left in END_LEFT:
            if end_shape(min(n, MEMBER), left):
                out["end_n%d_left%d" % (n, left)] = lambda seed, n=n, left=left: end_of_text(n, left, seed)
    out["step_geometry"] = step_geometry
    for lead in (0, 29):
        for dist in (32768, 32769):
            out["window_%d_lead%d" % (dist, lead)] = lambda seed, dist=dist, lead=lead: window(dist, lead, seed)
    out["too_far"] = too_far
    for k in ("run", "period2", "period3", "interleaved", "letter64", "lowest"):
        out["in_step_" + k] = lambda seed, k=k: in_step(k, seed)
    out["insert_order"] = insert_order
    out["hash_collision"] = hash_collision
    out["skewed_literals"] = skewed_literals
    out["skewed_distances"] = skewed_distances
    for a in KIND_ALPHABETS:
        for n in KIND_LENGTHS:
            out["kind_a%d_n%d" % (a, n)] = lambda seed, a=a, n=n: kind(a, n)
    out["member_boundary"] = member_boundary
    out["fastq"] = lambda seed: realistic()
    return out


def seed_name(name):
    return name.replace("window_32769", "window_32768")             # one stretch for both distances


def holds(text, check):
    try:
        check([R.parse_at(m) for m in R.members(text)], None)
        return True
    except AssertionError:
        return False


def search(name, build, limit=400):
    for seed in range(limit):
        if holds(*build(seed)):
            return seed
    raise AssertionError("no seed below %d gives %s its edge" % (limit, name))


def make_cases(find_seeds=False):
    out = collections.OrderedDict()
    for name, build in builders().items():
        key = seed_name(name)
        if find_seeds:
            SEEDS[key] = search(key, builders()[key])
        out[name] = Case(name, *build(SEEDS.get(key, 0)))
    return out


CASES = make_cases()
NAMES = list(CASES)
assert all(1 <= len(R.members(c.text)) <= 2 or c.name in ("member_boundary", "fastq") for c in CASES.values())

if __name__ == "__main__":
    SEEDS.clear()
    make_cases(find_seeds=True)
    print("SEEDS = {%s}" % ", ".join("%r: %d" % kv for kv in SEEDS.items() if kv[1]))
