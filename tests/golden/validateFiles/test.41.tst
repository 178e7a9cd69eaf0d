kreeq subgraph -d testFiles/random8.kreeq -f testFiles/random5.fasta 
embedded
Subgraph summary statistics:
Total kmers: 159
Unique kmers: 35
Distinct kmers: 97
Missing kmers: 4398046511007
Total edges: 165
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
# segments: 4
Total segment length: 177
Average segment length: 44.25
# gaps: 0
# paths: 0
# edges: 4
Average degree: 1.00
# connected components: 1
Largest connected component length: 177
# dead ends: 2
# disconnected components: 0
Total length disconnected components: 0
# separated components: 1
# bubbles: 0
# circular segments: 0
# circular paths: 0
DBG Summary statistics:
Total kmers: 159
Unique kmers: 35
Distinct kmers: 97
Missing kmers: 4398046511007
Total edges: 165
