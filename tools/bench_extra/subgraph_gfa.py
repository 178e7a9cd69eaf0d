"""Wall clock of kq_subgraph_gfa ("Measured: the graph"): the database and the contig of
tools/bench_extra/subgraph_bestfirst.py (100 Mbp shape, 30x 150 bp reads with 0.5 % substitutions, k = 21; a 1 Mbp contig of
the genome with 1e-4 substitutions), best-first at depth 21, trim, then the graph in both modes: the counts-only call and
the call that returns the arrays, by the host clock around the synchronising calls.  One run; a few lines.

    python tools/bench_extra/subgraph_gfa.py [genome_mbp] [contig_mbp] [depth]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch

from kreeq_amd import KreeqDB, capi, synth

G = int(float(sys.argv[1]) * 1e6) if len(sys.argv) > 1 else 100_000_000
CONTIG = int(float(sys.argv[2]) * 1e6) if len(sys.argv) > 2 else 1_000_000
COV, L, K, ERR, ASM_ERR, BATCH_READS = 30, 150, 21, 0.005, 1e-4, 5_000_000
DEPTH = int(sys.argv[3]) if len(sys.argv) > 3 else 21

dev = torch.device("cuda", 0)
n_reads = G * COV // L
genome = synth.genome_dev(G, dev, seed=1)
gen = torch.Generator(device=dev)
gen.manual_seed(2)
db = KreeqDB(K, 128, capacity_hint=int(1.1 * (G + n_reads * L * ERR * K)))
db.set_option("trust_capacity", 1)
t0 = time.perf_counter()
for lo in range(0, n_reads, BATCH_READS):
    batch = synth.reads_dev(genome, min(BATCH_READS, n_reads - lo), L, gen, err=ERR)
    torch.cuda.synchronize(dev)                        # the batch was made on torch's stream, the handle counts on its own
    db.count_batch_dev(batch.data_ptr(), batch.numel())
    torch.cuda.synchronize(dev)
    del batch
db.sync()
print(f"database: {db.summary()['distinct']} distinct k-mers of {n_reads} reads, counted in {time.perf_counter() - t0:.2f} s", flush=True)

contig_codes, _ = synth.mutate_dev(genome[G // 2:G // 2 + CONTIG].clone(), ASM_ERR, seed=3)
contig = synth.ascii_dev(contig_codes)
torch.cuda.synchronize(dev)
sub = KreeqDB(K, 128, capacity_hint=CONTIG + 1024)
db.subgraph_seed_dev(sub, contig.data_ptr(), contig.numel())
added = db.subgraph_best_first(sub, DEPTH, 0)
sub.subgraph_trim(0)
print(f"subgraph: {sub.summary()['distinct']} k-mers ({added} added by best-first at depth {DEPTH})", flush=True)


def rounds_of(handle):
    buf = C.create_string_buffer(1 << 14)
    rc = capi.load().kq_get_profile(handle.handle, buf, len(buf))
    return sum(kv.startswith("gfa_rank_") for kv in buf.value.decode().split(";")) if rc == 0 else -1


sub.set_option("profile", 1)
for no_collapse in (False, True):
    t0 = time.perf_counter()
    rc, counts, _, _, _ = sub.subgraph_gfa_raw(no_collapse)
    t1 = time.perf_counter()
    assert rc == 0, rc
    rounds = rounds_of(sub)
    t2 = time.perf_counter()
    segs, seq, edges, counts = sub.subgraph_gfa(no_collapse)         # (its own counts-only call included)
    t3 = time.perf_counter()
    print(f"gfa {'no-collapse' if no_collapse else 'collapsed'}: {counts['n_segments']} segments, {counts['n_seq']} bases, {counts['n_edges']} links, "
          f"{counts['n_dropped_edges']} dropped, {counts['n_cycles']} cycles, {rounds} ranking rounds: counts only {(t1 - t0) * 1e3:.2f} ms, "
          f"counts + arrays (two calls, numpy buffers allocated in between) {(t3 - t2) * 1e3:.2f} ms", flush=True)
sub.close()
db.close()
