kreeq subgraph -d testFiles/random10.kreeq -f testFiles/random5.fasta --search-depth 15 --traversal-algorithm traversal 
embedded
Subgraph summary statistics:
Total kmers: 157
Unique kmers: 61
Distinct kmers: 109
Missing kmers: 4398046510995
Total edges: 184
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
# segments: 5
Total segment length: 209
Average segment length: 41.80
# gaps: 0
# paths: 0
# edges: 4
Average degree: 0.80
# connected components: 1
Largest connected component length: 209
# dead ends: 4
# disconnected components: 0
Total length disconnected components: 0
# separated components: 1
# bubbles: 0
# circular segments: 0
# circular paths: 0
DBG Summary statistics:
Total kmers: 158
Unique kmers: 62
Distinct kmers: 110
Missing kmers: 4398046510994
Total edges: 188
