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
// -o x.kwig.gz / .bed.gz / .csvtable.gz (OutPlan::table_gz): the same text as a BGZF file -- on the device paths every formatted
// chunk is deflated there (kq_deflate_bgzf_dev), on the host path the writer's text goes through zlib (bgzf_out.h); the inflated
// bytes are the plain format's on every path, the compressed bytes differ between the two sides.
// Host: r.per_base was filled by the lookups of the map-range loop.
// Device (KQ_TABLE_DEVICE=1, off by default; a resident table and no sequence above kDeviceCallBytes): nothing has been looked
// up yet; the lookup keeps its per-base array on the GPU, which orients and formats it, and the QV table is printed at the end.
bool table_device_wanted(const Run& r);
void write_per_base_device(Run& r);
void write_per_base_host(const Run& r);

// Device, under map-range passes (KQ_TABLE_DEVICE=1 and KQ_TABLE_DEVICE_PASSES=1, off by default): the oriented triples of the
// whole genome accumulate in one device array over the ranges.  begin() plans (plan_table_passes, with KQ_TABLE_CALL_BYTES as
// the group limit) and takes the accumulator, one text buffer, one per-base array and the counters BEFORE the first fill, so
// that the count path sizes its arena around them; false -- a sequence above the limit, more than KQ_TABLE_ACC_MAX_BYTES, no
// memory -- leaves nothing allocated, logs the bytes and the reason, and the host path runs.  range() follows the fill of a
// range: per group copy, kq_lookup_sequence_dev over the range's maps, kq_per_base_merge_dev (which leaves the per-base array
// zero again).  write() reads the counters once and takes the accumulator to the file like write_per_base_device.
struct TablePasses {
    SegmentLists segs;
    TablePassPlan plan;
    uint32_t* d_acc = nullptr;
    char* d_text = nullptr;
    kq_dbgbase* d_pb = nullptr;
    uint64_t* d_ctr = nullptr;
    int n_ranges = 0;
    bool trace = false;                   // KQ_TABLE_TRACE=1
    double t_lookup = 0, t_merge = 0;
};
bool table_passes_wanted(const Run& r);
bool table_passes_begin(Run& r, TablePasses& t);
void table_passes_range(Run& r, TablePasses& t, int lo, int hi);
void table_passes_write(Run& r, TablePasses& t);

}  // namespace kqhost
