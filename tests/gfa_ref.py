"""CPU restatement of the graph `kreeq subgraph` hands to its GFA writer (reference DBG::DBGgraphToGFA and DBG::collapseNodes,
src/kreeq.cpp:360-600) -- TEST INFRASTRUCTURE ONLY.

Pure Python on the trimmed subgraph table {key: (fw[4], bw[4], cov)} of tests/subgraph_ref.py.  The reference collapses with
one thread that erases from a hash map while it iterates it (:429-461): node numbers, the k-mer whose cov becomes DP (:458) and
the order of the links are the map's order, and on asymmetric counters so is the outcome ("at most one back edge", :412).  The
rules here are the order-free ones that give the numbers of the reference's goldens (tests/test_gfa_ref.py):

  oriented k-mers   (x,+) = the canonical string of key x, (x,-) its reverse complement; id = 2 * rank of x + (o == '-')
  out-edges         of (x,+): the non-zero fw[i] (:468-491, :549-570), of (x,-): the non-zero bw[i], mirrored (:493-517, :571-593)
  link              v -> w: v has exactly one out-edge (:377-383, :437), w's key is present and another one, no key is its own
                    reverse complement, and flip(w) has exactly one out-edge, which leads to flip(v)   (mutual form of :412)
  chains            of links; a cycle pair is cut in front of the smallest oriented id of both cycles (and behind its flip in the
                    mirror cycle, so that the two stay mirrors); of a mirror pair the chain with the smaller head id is kept
  segments          one per kept chain, numbered by ascending head id; head k-mer + last base of every following one (:417, :457)
  DP                cov of the head k-mer (:458 prints the cov of the k-mer the walk started from); no CB tag (no colour kept)
  edges             collapsed: out-edges that are no links and whose target is present; emitted when the target is the first
                    k-mer of its chain, else dropped (n_dropped_edges); of an edge and its mirror the smaller (source, target)
                    --no-collapse: the two line forms of :549-593, nothing deduplicated
"""
import types

from tests.subgraph_ref import next_key

ITOC = "ACGT"
NONE = -1


def kmer_string(key, k):
    """reverseHash: keys hold the first base in the low bits"""
    return "".join(ITOC[(key >> (2 * c)) & 3] for c in range(k))


def revcomp(s):
    return "".join(ITOC[3 - ITOC.index(c)] for c in reversed(s))


def oriented_string(keys, v, k):
    s = kmer_string(keys[v >> 1], k)
    return revcomp(s) if v & 1 else s


def out_edges(table, keys, rank, v, k):
    """-> [(base index, counter, target oriented id or NONE when the neighbour is absent)]"""
    x = keys[v >> 1]
    fw, bw, _ = table[x]
    out = []
    for i in range(4):
        c = bw[i] if v & 1 else fw[i]
        if c == 0:
            continue
        y, is_fw = next_key(x, i, not (v & 1), k)
        if y not in rank:
            out.append((i, c, NONE))
        else:
            minus = (not is_fw) if not (v & 1) else is_fw               # (x,+): '+' iff isFw; (x,-): '-' iff isFw
            out.append((i, c, 2 * rank[y] + int(minus)))
    return out


def _palindrome(key, k):
    s = kmer_string(key, k)
    return s == revcomp(s)


def build(table, k, no_collapse=False):
    """-> namespace(segs = [(seq_off, head_key, n_kmers, cov, head_rc)], seq = str, edges = [(from, to, count, from_rc, to_rc)],
    counts = {n_segments, n_seq, n_edges, n_dropped_edges, n_cycles}, rounds = pointer-jumping rounds a doubling scheme needs)"""
    keys = sorted(table)
    rank = {x: r for r, x in enumerate(keys)}
    n = len(keys)
    segs, seq, edges = [], [], []
    n_dropped = n_cycles = 0
    if no_collapse:
        off = 0
        for r, x in enumerate(keys):
            segs.append((off, x, 1, table[x][2], 0))
            seq.append(kmer_string(x, k))
            off += k
        for r, x in enumerate(keys):
            for i, c, w in out_edges(table, keys, rank, 2 * r, k):      # this + -> next (isFw ? + : -)
                if w != NONE:
                    edges.append((r, w >> 1, c, 0, w & 1))
            for i, c, w in out_edges(table, keys, rank, 2 * r + 1, k):  # prev (isFw ? + : -) -> this +: the flip of (x,-) -> w
                if w != NONE:
                    edges.append((w >> 1, r, c, (w & 1) ^ 1, 0))
    else:
        outs = [out_edges(table, keys, rank, v, k) for v in range(2 * n)]
        pal = [_palindrome(x, k) for x in keys]
        succ = [NONE] * (2 * n)
        for v in range(2 * n):
            if len(outs[v]) != 1:
                continue
            w = outs[v][0][2]
            if w == NONE or (w >> 1) == (v >> 1) or pal[v >> 1] or pal[w >> 1]:
                continue
            back = outs[w ^ 1]
            if len(back) == 1 and back[0][2] == (v ^ 1):
                succ[v] = w
        pred = [NONE] * (2 * n)
        for v in range(2 * n):
            if succ[v] != NONE:
                assert pred[succ[v]] == NONE
                pred[succ[v]] = v
        # cycles: what no walk back from a node without predecessor reaches
        seen = [False] * (2 * n)
        for v in range(2 * n):
            if pred[v] == NONE:
                while v != NONE:
                    seen[v] = True
                    v = succ[v]
        cyc_min = {}
        for v in range(2 * n):
            if not seen[v] and v not in cyc_min:
                members, u = [v], succ[v]
                while u != v:
                    members.append(u)
                    u = succ[u]
                for u in members:
                    cyc_min[u] = min(members)
        for m in sorted(set(cyc_min.values())):
            if m < cyc_min[m ^ 1]:                                      # the kept cycle of the pair: cut in front of m
                p = pred[m]
                succ[p] = NONE
                pred[m] = NONE
                pred[succ[m ^ 1]] = NONE                                # flip(m) -> flip(p), the mirror of the cut link
                succ[m ^ 1] = NONE
                n_cycles += 1
        head, dist = [NONE] * (2 * n), [0] * (2 * n)
        for v in range(2 * n):
            if pred[v] == NONE:
                u, d = v, 0
                while u != NONE:
                    head[u], dist[u] = v, d
                    u, d = succ[u], d + 1
        assert NONE not in head
        kept = [head[v] < head[v ^ 1] for v in range(2 * n)]
        seg_of, off = {}, 0
        for h in range(2 * n):
            if head[h] == h and kept[h]:
                seg_of[h] = len(segs)
                s, u = oriented_string(keys, h, k), succ[h]
                while u != NONE:
                    s += oriented_string(keys, u, k)[-1]
                    u = succ[u]
                segs.append((off, keys[h >> 1], len(s) - k + 1, table[keys[h >> 1]][2], h & 1))
                seq.append(s)
                off += len(s)

        def end_of(u):                                                  # (segment, rc) of an oriented k-mer at a chain end
            return (seg_of[head[u]], 0) if kept[u] else (seg_of[head[u ^ 1]], 1)

        for v in range(2 * n):
            for i, c, w in outs[v]:
                if w == NONE or succ[v] == w:
                    continue
                assert succ[v] == NONE                                  # v is the last k-mer of its chain
                if head[w] != w:
                    n_dropped += 1
                    continue
                mirror = any(t == (v ^ 1) for _, _, t in outs[w ^ 1])
                if mirror and (w ^ 1, v ^ 1) < (v, w):
                    continue
                a, b = end_of(v), end_of(w)
                edges.append((a[0], b[0], c, a[1], b[1]))
    longest = max([s[2] for s in segs], default=0)
    counts = {"n_segments": len(segs), "n_seq": sum(len(s) for s in seq), "n_edges": len(edges), "n_dropped_edges": n_dropped,
              "n_cycles": n_cycles}
    return types.SimpleNamespace(k=k, segs=segs, seq="".join(seq), edges=edges, counts=counts, longest=longest)


def segment_strings(g):
    return [g.seq[off:off + n + g.k - 1] for off, _, n, _, _ in g.segs]


def gfa_text(g):
    lines = ["H\tVN:Z:1.0"]
    for i, (s, seg) in enumerate(zip(segment_strings(g), g.segs)):
        lines.append(f"S\t{i}\t{s}\tDP:f:{seg[3]}")
    for a, b, c, arc, brc in g.edges:
        lines.append(f"L\t{a}\t{'-' if arc else '+'}\t{b}\t{'-' if brc else '+'}\t{g.k - 1}M\tKC:i:{c}")
    return "\n".join(lines) + "\n"


def stats(g):
    """the computed lines of the block: union-find over the emitted links, touched segment ends"""
    n = len(g.segs)
    lens = [s[2] + g.k - 1 for s in g.segs]
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    touched, circular = set(), set()
    for a, b, _, arc, brc in g.edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
        touched.add((a, 0 if arc else 1))                               # side 1 = the '+' end, side 0 = the '+' start
        touched.add((b, 1 if brc else 0))
        if a == b and arc == brc:
            circular.add(a)
    comp = {}
    for i in range(n):
        comp[find(i)] = comp.get(find(i), 0) + lens[i]
    lonely = [i for i in range(n) if (i, 0) not in touched and (i, 1) not in touched]
    return {"segments": n, "total_len": sum(lens), "edges": len(g.edges), "components": len(comp), "largest": max(comp.values(), default=0),
            "dead_ends": 2 * n - len(touched), "disconnected": len(lonely), "disconnected_len": sum(lens[i] for i in lonely),
            "circular": len(circular)}


def _ratio(a, b):
    return "nan" if b == 0 else "%.2f" % (a / b)


def block_lines(g):
    """the "+++Assembly summary+++" block in the reference's layout, without `# separated components` and `# bubbles`"""
    s = stats(g)
    return ["+++Assembly summary+++: ", "# scaffolds: 0", "Total scaffold length: 0", "Average scaffold length: nan", "Scaffold N50: 0",
            "Scaffold auN: 0.00", "Scaffold L50: 0", "Largest scaffold: 0", "Smallest scaffold: 0", "# contigs: 0", "Total contig length: 0",
            "Average contig length: nan", "Contig N50: 0", "Contig auN: 0.00", "Contig L50: 0", "Largest contig: 0", "Smallest contig: 0",
            "# gaps in scaffolds: 0", "Total gap length in scaffolds: 0", "Average gap length in scaffolds: 0.00", "Gap N50 in scaffolds: 0",
            "Gap auN in scaffolds: 0.00", "Gap L50 in scaffolds: 0", "Largest gap in scaffolds: 0", "Smallest gap in scaffolds: 0",
            "Base composition (A:C:G:T): 0:0:0:0", "GC content %: nan", "# soft-masked bases: 0",
            f"# segments: {s['segments']}", f"Total segment length: {s['total_len']}",
            f"Average segment length: {_ratio(s['total_len'], s['segments'])}", "# gaps: 0", "# paths: 0", f"# edges: {s['edges']}",
            f"Average degree: {_ratio(s['edges'], s['segments'])}", f"# connected components: {s['components']}",
            f"Largest connected component length: {s['largest']}", f"# dead ends: {s['dead_ends']}",
            f"# disconnected components: {s['disconnected']}", f"Total length disconnected components: {s['disconnected_len']}",
            f"# circular segments: {s['circular']}", "# circular paths: 0"]


UNPRINTED = ("# separated components: ", "# bubbles: ")


def golden_block(lines):
    """the block of a golden (.tst expected lines) without the two lines this build does not print"""
    a, b = lines.index("+++Assembly summary+++: "), lines.index("DBG Summary statistics:")
    return [x for x in lines[a:b] if not x.startswith(UNPRINTED)]
