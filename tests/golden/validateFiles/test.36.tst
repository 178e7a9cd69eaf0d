kreeq subgraph -d testFiles/test1.kreeq -f testFiles/random1.fasta --search-depth 0 --no-collapse 
embedded
Subgraph summary statistics:
Total kmers: 1156
Unique kmers: 168
Distinct kmers: 260
Missing kmers: 4398046510844
Total edges: 446
+++Assembly summary+++: 
# scaffolds: 0
Total scaffold length: 0
Average scaffold length: nan
Scaffold N50: 0
Scaffold auN: 0.00
Scaffold L50: 0
Largest scaffold: 0
Smallest scaffold: 0
# contigs: 0
Total contig length: 0
Average contig length: nan
Contig N50: 0
Contig auN: 0.00
Contig L50: 0
Largest contig: 0
Smallest contig: 0
# gaps in scaffolds: 0
Total gap length in scaffolds: 0
Average gap length in scaffolds: 0.00
Gap N50 in scaffolds: 0
Gap auN in scaffolds: 0.00
Gap L50 in scaffolds: 0
Largest gap in scaffolds: 0
Smallest gap in scaffolds: 0
Base composition (A:C:G:T): 0:0:0:0
GC content %: nan
# soft-masked bases: 0
# segments: 260
Total segment length: 5460
Average segment length: 21.00
# gaps: 0
# paths: 0
# edges: 520
Average degree: 2.00
# connected components: 1
Largest connected component length: 5460
# dead ends: 2
# disconnected components: 0
Total length disconnected components: 0
# separated components: 1
# bubbles: 0
# circular segments: 0
# circular paths: 0
DBG Summary statistics:
Total kmers: 172
Unique kmers: 25
Distinct kmers: 96
Missing kmers: 4398046511008
Total edges: 160
