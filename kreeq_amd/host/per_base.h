// per_base.h -- the state of one CLI run and the outputs of a validation: the QV table and the four per-base files.
#pragma once
#include "cli_common.h"
#include "cli_plan.h"

namespace kqhost {

struct Run {
    kq_handle* h = nullptr;               // the table (one map range of it at a time under --passes / -m)
    UserInput ui;
    OutPlan plan;
    int k = 21, map_count = 128;
    std::vector<SeqRecord> seqs;          // -f (reference Input::loadGenome, src/input.cpp:188-308) ...
    JoinedSeqs genome;                    // ... and its text as the lookups take it
    std::vector<kq_dbgbase> per_base;     // aligned with genome.text when a host writer needs it
    uint64_t counters[3] = {0, 0, 0};     // missing, evaluated, edge-missing: add up over map ranges and device calls
};

void print_qv(const Run& r);              // src/kreeq.cpp:78-106; prints nothing for a -o name without a dot

// -o x.kwig / .bkwig / .bed / .csvtable, by whichever side may write them; every byte is the same.
// Host: r.per_base was filled by the lookups of the map-range loop.
// Device (KQ_TABLE_DEVICE=1, off by default; a resident table and no sequence above kDeviceCallBytes): nothing has been looked
// up yet; the lookup keeps its per-base array on the GPU, which orients and formats it, and the QV table is printed at the end.
bool table_device_wanted(const Run& r);
void write_per_base_device(Run& r);
void write_per_base_host(const Run& r);

}  // namespace kqhost
