"""CPU restatement of kreeq's `subgraph` mode (reference src/subgraph.cpp) -- TEST INFRASTRUCTURE ONLY.

Pure Python on {key: (fw[4], bw[4], cov)} tables; every function cites the reference lines it follows.
  seed          DBG::subgraph + DBGsubgraphFromSegment + mergeSubgraphs   src/subgraph.cpp:116-161, :190-288, :42-112
  traversal     DBG::traversal + traversalPass                           :301-415   (single map range)
  best_first    DBG::bestFirst + dijkstra                                :417-579   (single map range)
  trim          DBG::removeMissingEdges                                  :599-628
  summary       DBG::summary(ParallelMap32color&)                        :163-188
Pinned by tests/test_subgraph_ref.py against validateFiles/test.36.tst .. test.47.tst.
"""
import numpy as np

from oracle.variants import CTOI, FibHeap

LARGEST = 2 ** 32 - 1                                                    # include/kreeq.h:68


def table_of(entries):
    """helpers.load_db_table / an export (structured array) -> {key: (fw, bw, cov)}"""
    return {int(e["key"]): ([int(x) for x in e["fw"]], [int(x) for x in e["bw"]], int(e["cov"])) for e in entries}


def entries_of(table):
    """{key: (fw, bw, cov)} -> structured array sorted by key, hc as the engine exports it (cov >= 255)"""
    dt = np.dtype([("key", "<u8"), ("fw", "<u4", 4), ("bw", "<u4", 4), ("cov", "<u4"), ("hc", "<u4")])
    return np.array([(key, v[0], v[1], v[2], int(v[2] >= 255)) for key, v in sorted(table.items())], dtype=dt)


def segments_of(seq):
    """the ACGT runs of a byte string or str (gfalibs splits at N; any other byte ends a run here as well)"""
    if isinstance(seq, (bytes, bytearray)):
        seq = seq.decode("latin-1")
    out, i = [], 0
    while i < len(seq):
        if seq[i] not in CTOI:
            i += 1
            continue
        j = i
        while j < len(seq) and seq[j] in CTOI:
            j += 1
        out.append(seq[i:j])
        i = j
    return out


def next_key(key, base, fw, k):
    """DBG::buildNextKmer + hash, :581-597: a fw edge appends `base` to the canonical string, a bw edge prepends it
    -> (canonical key, isFw); keys hold the first base in the low bits"""
    mask = (1 << (2 * k)) - 1
    nxt = ((key >> 2) | (base << (2 * k - 2))) if fw else (((key << 2) | base) & mask)
    rv = 0
    for c in range(k):
        rv |= (3 - ((nxt >> (2 * c)) & 3)) << (2 * (k - 1 - c))
    return (nxt, True) if nxt < rv else (rv, False)


def seed(db, seqs, k, no_reference=False):
    """:190-288 per segment, then the saturating sum of :42-112.  seqs: iterable of sequences (bytes / str)."""
    sub = {}
    mask = (1 << (2 * k)) - 1
    for seq in seqs:
        for seg in segments_of(seq):
            n = len(seg)
            if n < k:                                                    # :204
                continue
            codes = [CTOI[c] for c in seg]
            seg_map = {}
            fwd = rev = 0
            for end in range(n):
                fwd = (fwd >> 2) | (codes[end] << (2 * k - 2))
                rev = ((rev << 2) | (3 - codes[end])) & mask
                if end < k - 1:
                    continue
                p = end - k + 1
                key, is_fw = (fwd, True) if fwd < rev else (rev, False)
                if key in seg_map:                                       # insert() keeps the first (:242, :276)
                    continue
                if key in db:                                            # :238-249 (either tier: exact counters)
                    f, b, cov = db[key]
                    seg_map[key] = (list(f), list(b), cov)
                elif not no_reference:                                   # :250-277
                    f, b = [0] * 4, [0] * 4
                    nxt = codes[p + k] if p + k < n else 4
                    prv = codes[p - 1] if p > 0 else 4
                    if is_fw:
                        if nxt <= 3:
                            f[nxt] = 1
                        if prv <= 3:
                            b[prv] = 1
                    else:
                        if prv <= 3:
                            f[3 - prv] = 1
                        if nxt <= 3:
                            b[3 - nxt] = 1
                    seg_map[key] = (f, b, 1)
            for key, (f, b, cov) in seg_map.items():                     # :58-85
                if key not in sub:
                    sub[key] = (list(f), list(b), cov)
                else:
                    sf, sb, sc = sub[key]
                    sub[key] = ([min(LARGEST, x + y) for x, y in zip(sf, f)], [min(LARGEST, x + y) for x, y in zip(sb, b)],
                                min(LARGEST, sc + cov))
    return sub


def traversal(db, sub, k, depth):
    """:301-415.  Round 1 starts from the seeds, round r + 1 from what round r found; candidates are tested against
    the seed set only and inserted at the end without overwriting.  -> number of k-mers added"""
    seeds = sub
    candidates = {}
    frontier = sub
    for _ in range(depth):                                               # :307
        new = {}
        for key, (f, b, _) in frontier.items():
            for fw, counts in ((True, f), (False, b)):                   # :330, :371
                for i in range(4):
                    if counts[i] != 0:
                        nk, _ = next_key(key, i, fw, k)
                        if nk not in seeds and nk in db and nk not in new:
                            new[nk] = db[nk]
        for nk, v in new.items():                                        # :317
            candidates.setdefault(nk, v)
        frontier = new                                                   # :318
    added = 0
    for nk, v in candidates.items():                                     # :321
        if nk not in sub:
            sub[nk] = (list(v[0]), list(v[1]), v[2])
            added += 1
    return added


def _dijkstra(db, seeds, source, k, depth, cov_cutoff):
    """:460-579 for one source -> the k-mers on the prev chains of its destinations (source excluded)"""
    Q = FibHeap()
    dist = {source: 1}                                                   # :469
    prev = {}
    Q.insert(source, 1)                                                  # :471
    d = 0
    direction = True
    destinations = []
    while Q.size() > 0 and d < depth + 1:                                # :477
        u = Q.extract_min()                                              # :482
        if u in prev:                                                    # :483-486
            direction = prev[u][1]
        f, b, _ = seeds[source] if u == source else db[u]                # the source carries its merged subgraph entry (:470)

        def check_next(key, dirn):                                       # :488-518
            if key in seeds:
                return
            if key not in db:                                            # the reference dereferences end() here: not followed
                return
            alt = dist[u]
            if alt < 255:
                alt += 1
            if key not in dist:
                dist[key] = 255
                Q.insert(key, 0)
            if alt < dist[key]:
                prev[key] = (u, dirn)
                dist[key] = alt
                Q.decrease_key(key, alt)                                 # a no-op: alt > 0 (include/fibonacci-heap.h:141)

        for i in range(4):                                               # :520-558
            if direction or d == 0:
                if d == 0:
                    direction = True
                if f[i] > cov_cutoff:
                    key, is_fw = next_key(u, i, True, k)
                    check_next(key, direction if is_fw else not direction)
                    if key in seeds:
                        destinations.append(u)
            if (not direction) or d == 0:
                if d == 0:
                    direction = False
                if b[i] > cov_cutoff:
                    key, is_fw = next_key(u, i, False, k)
                    check_next(key, direction if is_fw else not direction)
                    if key in seeds:
                        destinations.append(u)
        d += 1
    found = set()
    for node in destinations:                                            # :563-570
        while node != source and node not in found:
            found.add(node)
            if node not in prev:                                         # (a chain of 254 nodes saturates dist: no prev)
                break
            node = prev[node][0]
    return found


def best_first(db, sub, k, depth, cov_cutoff=0):
    """:417-458: one search per seed (one map range: always explored), discoveries inserted without overwriting"""
    seeds = dict(sub)
    found = set()
    for source in seeds:
        found |= _dijkstra(db, seeds, source, k, depth, cov_cutoff)
    added = 0
    for key in found:
        if key not in sub:
            sub[key] = (list(db[key][0]), list(db[key][1]), db[key][2])
            added += 1
    return added


def trim(sub, k, cov_cutoff=0):
    """:599-625: counters > cutoff whose neighbour is outside the subgraph become 0 (smaller ones are not looked at)"""
    for key, (f, b, _) in sub.items():
        for i in range(4):
            if f[i] > cov_cutoff and next_key(key, i, True, k)[0] not in sub:
                f[i] = 0
            if b[i] > cov_cutoff and next_key(key, i, False, k)[0] not in sub:
                b[i] = 0


def summary(sub, k):
    """:163-188, with the precedence of :174: fw > 0 ? 1 : (bw > 0 ? 1 : 0)"""
    edges = sum((1 if f[w] > 0 else (1 if b[w] > 0 else 0)) for f, b, _ in sub.values() for w in range(4))
    return {"total": sum(v[2] for v in sub.values()), "unique": sum(v[2] == 1 for v in sub.values()), "distinct": len(sub),
            "missing": 4 ** k - len(sub), "edges": edges}


def subgraph(db, seqs, k, depth=None, algorithm="best-first", no_reference=False, cov_cutoff=0):
    """the flow of src/input.cpp:153-181 up to the summary -> the trimmed subgraph table"""
    if depth is None:                                                    # include/kreeq.h:171-175
        depth = k if algorithm == "best-first" else (k + 1) // 2
    sub = seed(db, seqs, k, no_reference)
    if algorithm == "best-first":
        best_first(db, sub, k, depth, cov_cutoff)
    elif algorithm == "traversal":
        traversal(db, sub, k, depth)
    else:
        raise ValueError(algorithm)
    trim(sub, k, cov_cutoff)
    return sub
