// The output plan of the compressed per-base tables (kreeq_amd/host/cli_plan.h) as a stand-alone host program: x.kwig.gz,
// x.bed.gz and x.csvtable.gz set table_gz and name the format inside, without becoming per_base files or losing their ".gz";
// x.bkwig.gz, x.gfa.gz and the plain names do not.
#include <cstdio>
#include <string>

#include "cli_plan.h"

using namespace kqhost;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

struct Row { int mode; const char* out; const char* ext; int table_gz; const char* table_ext; int per_base, tables, refused; const char* format; };
static const Row kRows[] = {
    {0, "x.kwig.gz", "kwig.gz", 1, "kwig", 0, 1, 0, "kwig"},
    {0, "x.bed.gz", "bed.gz", 1, "bed", 0, 1, 0, "bed"},
    {0, "x.csvtable.gz", "csvtable.gz", 1, "csvtable", 0, 1, 0, "csvtable"},
    {0, "dir.d/run.1.kwig.gz", "kwig.gz", 1, "kwig", 0, 1, 0, "kwig"},
    {0, "x.bkwig.gz", "bkwig.gz", 0, "", 0, 0, 0, "bkwig.gz"},          // binary and compact already: not a format
    {0, "x.gfa.gz", "gfa.gz", 0, "", 0, 0, 1, "gfa.gz"},
    {0, "x.vcf.gz", "vcf.gz", 0, "", 0, 0, 0, "vcf.gz"},
    {0, "x.kwig", "kwig", 0, "", 1, 1, 0, "kwig"},
    {0, "x.bed", "bed", 0, "", 1, 1, 0, "bed"},
    {0, "x.csvtable", "csvtable", 0, "", 1, 1, 0, "csvtable"},
    {0, "x.bkwig", "bkwig", 0, "", 1, 1, 0, "bkwig"},
    {0, "", "stdout", 0, "", 0, 0, 0, "stdout"},
};

int main() {
    for (const Row& w : kRows) {
        const OutPlan p = plan_output(w.mode, w.out);
        CHECK(p.ext == w.ext, "-o '%s': ext '%s'", w.out, p.ext.c_str());
        CHECK(p.table_gz == !!w.table_gz && p.table_ext == w.table_ext, "-o '%s': table_gz %d table_ext '%s'", w.out, p.table_gz, p.table_ext.c_str());
        CHECK(p.per_base == !!w.per_base && p.tables() == !!w.tables && p.refused == !!w.refused, "-o '%s': per_base %d tables %d refused %d", w.out, p.per_base,
              p.tables(), p.refused);
        CHECK(p.table_format() == w.format, "-o '%s': format '%s'", w.out, p.table_format().c_str());
        CHECK(p.want_stats && p.want_qv && !p.vcf && !p.kreeq && !p.hist, "-o '%s': the summary and the QV table, nothing else", w.out);
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
