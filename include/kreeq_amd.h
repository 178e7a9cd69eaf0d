/*
 * kreeq_amd.h -- C ABI of the MI355X-native k-mer count / QV engine (libkreeq_amd.so).
 *
 * This is the drop-in boundary for kreeq's hot path.  kreeq has no plugin / FFI interface; the
 * seams a replacement sits behind are the CRTP hooks gfalibs' Kmap calls on DBG.
 * Each entry point below names the reference hook it replaces (paths relative to the reference
 * repository vgl-hub/kreeq @ 2024_08_07).  INTEGRATION.md shows the binding a kreeq maintainer
 * would add inside those hooks.
 *
 * Conventions
 *   - every function returns 0 (KQ_OK) or a negative kq_status; kq_last_error() returns a
 *     thread-local message for the last failure on the calling thread; no C++ exception and no
 *     torch type ever crosses this boundary;
 *   - one handle per GPU; calls on one handle must be serialised by the caller, different handles
 *     may be used from different threads / processes concurrently;
 *   - plain pointers and sizes only.  "host" entry points take host buffers and copy over PCIe;
 *     the *_dev entry points take device pointers valid on the handle's GPU and are asynchronous
 *     on the handle's stream (kq_sync() / any host-returning call synchronises);
 *   - a "read batch" / "sequence" is a byte string of bases; any byte other than ACGTacgt ends
 *     the current run, so reads inside a batch are separated by one such byte (e.g. '\n' or 'N')
 *     and k-mers never span it -- exactly the reference's behaviour on a bad base
 *     (src/graph-builder.cpp:77-91) and gfalibs' splitting of assembly sequences at N.
 *
 * There is no CPU fallback: every compute entry point fails with KQ_ERR_NO_DEVICE when no gfx950
 * device is usable.
 */
#ifndef KREEQ_AMD_H
#define KREEQ_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KQ_ABI_VERSION 4

typedef enum {
    KQ_OK = 0,
    KQ_ERR_INVALID = -1,     /* bad argument (k, map_count, null pointer, map range ...) */
    KQ_ERR_NO_DEVICE = -2,   /* no usable HIP device / kernel image for this GPU */
    KQ_ERR_HIP = -3,         /* a HIP runtime call failed; message has the HIP error string */
    KQ_ERR_NOMEM = -4,       /* device or host allocation failed */
    KQ_ERR_TABLE_FULL = -5,  /* k-mer table (or its high-copy side table) could not grow */
    KQ_ERR_CAPACITY = -6,    /* caller's output buffer too small (n_out holds the needed size) */
    KQ_ERR_MISMATCH = -7     /* handles disagree on k / map_count / device */
} kq_status;

typedef struct kq_handle kq_handle;

/* Logical table entry == one k-mer of the de Bruijn graph with exact counters.
 * Replaces the value types DBGkmer / DBGkmer32 (include/kreeq.h:20-21, :69-70): hc != 0 marks a
 * k-mer that the reference keeps in the 32-bit high-copy map (cov >= 255), hc == 0 one whose
 * counters all fit the 8-bit map.  Counters saturate at 2^32-1 (LARGEST, include/kreeq.h:68). */
typedef struct {
    uint64_t key;
    uint32_t fw[4], bw[4], cov;
    uint32_t hc;
} kq_entry;

/* Per-position validation result == DBGbase (include/input.h:4-9). */
typedef struct {
    uint32_t fw, bw, cov;
    uint8_t  isFw;
    uint8_t  pad[3];
} kq_dbgbase;

/* Numbers of the "DBG Summary statistics" block (DBG::summary + DBG::DBstats,
 * src/graph-builder.cpp:240-295), including the ":254/:263" edge-count precedence quirk. */
typedef struct {
    uint64_t total;     /* Total kmers    */
    uint64_t unique;    /* Unique kmers   */
    uint64_t distinct;  /* Distinct kmers */
    uint64_t missing;   /* Missing kmers = 4^k - distinct */
    uint64_t edges;     /* Total edges    */
} kq_stats;

/* Running totals of one handle (not part of the reference; used for throughput reporting). */
typedef struct {
    uint64_t kmers_counted;   /* k-mer instances inserted so far (sum of cov added)          */
    uint64_t slots_used;      /* occupied table slots == distinct k-mers                      */
    uint64_t slots_total;     /* table capacity in slots                                      */
    uint64_t hc_used;         /* occupied high-copy side-table slots                          */
    uint64_t hc_total;
    uint64_t table_bytes;     /* HBM bytes held by table + side table                         */
    uint64_t table_passes;    /* region-wise passes over the table so far (see KQ_OPT_PENDING_BYTES) */
} kq_info;

/* ---- lifetime ---------------------------------------------------------------------------- */

/* Replaces the DBG / Kmap constructor (include/kreeq.h:168-177): k = kmerLen (2..32), map_count =
 * gfalibs mapCount (128 in every .kreeq .index).  capacity_hint = expected distinct k-mers
 * (0 = small default; the table grows by rehashing when needed). */
int  kq_create(kq_handle** out, int device, int k, int map_count, uint64_t capacity_hint);
void kq_destroy(kq_handle* h);
/* Drop all k-mers, keep the allocation. */
int  kq_clear(kq_handle* h);
/* Make the handle enqueue on a caller-owned hipStream_t (NULL = the handle's own stream). */
int  kq_set_stream(kq_handle* h, void* hip_stream);
void* kq_get_stream(kq_handle* h);
/* Tuning knobs (no reference counterpart).
 *   KQ_OPT_TRUST_CAPACITY  value != 0: capacity_hint given to kq_create is an upper bound of the
 *                          distinct k-mers the table will ever hold, so batches do not pre-grow the
 *                          table for their worst case (all k-mers new).  If the bound is wrong a
 *                          table region overflows and the next sync returns KQ_ERR_TABLE_FULL.
 *   KQ_OPT_COUNT_PATH      0 = auto, 1 = direct (global atomics), 2 = partitioned (LDS regions)
 *   KQ_OPT_SLICE_KMERS     k-mer starts processed per internal slice of a resident batch (default 2^28;
 *                          the partition scratch is 16 bytes per start)
 *   KQ_OPT_COUNT_MAP_RANGE value = lo | hi << 16: kq_count_batch(_dev) keeps only k-mers whose map index
 *                          key % map_count lies in [lo, hi).  This is the reference's memory-bounded mode
 *                          (process the maps in ranges, src/kreeq.cpp:59-74; README "HPC" runs + union):
 *                          count the same reads once per range into separate databases, then union.
 *   KQ_OPT_PROFILE         value != 0: HIP events are recorded around the stages of the partitioned count;
 *                          kq_get_profile() returns "stage=ms;..." for the last batch (measurement aid)
 *   KQ_OPT_LOOKUP_PATH     kq_lookup_sequence(_dev) without per-base output: 0 = auto, 1 = direct (one table probe
 *                          per k-mer), 2 = partitioned (the k-mers are split by table region like read k-mers
 *                          and evaluated against region images staged in LDS)
 *   KQ_OPT_MERGE_PATH      kq_merge into this handle: 0 = auto, 1 = one atomic add per source entry, 2 = region by
 *                          region (destination images staged in LDS, both tables streamed once)
 *   KQ_OPT_NARROW_MID      (tuning / tests) regions per hash-prefix bucket from which the record split of the
 *                          partitioned paths gets a middle level (default 2048, i.e. tables above 8.6 GB)
 *   KQ_OPT_PENDING_BYTES   the partitioned count keeps the region-sorted records of a slice PENDING in an arena of at most
 *                          this many bytes of HBM and applies all pending sets in one pass over the table (when the arena
 *                          is full, and before anything reads the table: kq_sync, summary, lookup, export, merge ...), so
 *                          that a large table is streamed once per arena-full of records rather than once per slice.
 *                          -1 = automatic (default: a few times the table, at most the free HBM less 1/8 of the device),
 *                          0 = apply every slice at once.  Results never depend on it (counting is commutative).
 *   KQ_OPT_BUCKET_WINDOW   value = lo | hi << 16, 0 <= lo < hi <= 256, on an EMPTY handle with k <= 21: the handle becomes one
 *                          shard of a multi-GPU database -- it holds, and answers for, only the k-mers whose table hash
 *                          starts with one of the 8-bit prefixes ("hash-prefix buckets") lo .. hi-1.  The memory kq_create
 *                          sized is kept and laid out as that window of a table 256 / (hi - lo) times larger, so the bucket
 *                          split of the count path is the owner split of the exchange (kq_emit_sharded_dev /
 *                          kq_insert_sharded_dev).  k-mers of other buckets are ignored by every entry point: counts drop
 *                          them, lookups do not evaluate them (their sum over the shards is the whole answer, like the map
 *                          ranges of src/kreeq.cpp:150), export / summary see the window's k-mers.
 *                          (KQ_OPT_SHARD_WINDOW is its superset: the same for k <= 21, and k = 29..32 as well.)
 *   KQ_OPT_SHARD_WINDOW    value = lo | hi << 16: KQ_OPT_BUCKET_WINDOW with every one of its rules (empty handle, 0 <= lo < hi <=
 *                          256, an empty windowed table moves to a window of the same width without a new allocation, [0, 256)
 *                          gives an ordinary table again), accepted for k <= 21 -- the same code path -- AND for k = 29..32,
 *                          whose tables have the 256-bucket geometry at every size (a slot there stores the 56 hash bits below
 *                          the bucket prefix; the prefix is implied by the slot's region of the whole geometry, windowed or not).
 *                          The shard of kq_emit_sharded8_dev / kq_insert_sharded8_dev.  k = 22..28 is refused: those shards
 *                          own map ranges (kq_emit_packed_dev). */
/*   KQ_OPT_OVERLAP        1 (default): a count call that cuts its batch into several slices (KQ_OPT_SLICE_KMERS) runs the
 *                          partition stages of consecutive slices on two internal streams with a scratch set each (slice
 *                          j+1's scan beside slice j's split levels) and joins them with the handle's stream before it
 *                          returns: the caller's stream-ordered view of the handle is unchanged.  0: one stream.
 *                          2: also in a map-range pass (KQ_OPT_COUNT_MAP_RANGE), where 1 does not fork (tests). */
/*   KQ_OPT_COUNT_MAP_PASSES n = 2, 4 or 8 (1 = off): the caller counts the SAME RESIDENT batches once per range of the equal split of
 *                          the maps into n (KQ_OPT_COUNT_MAP_RANGE = [r mapCount / n, (r + 1) mapCount / n), any order) and vouches
 *                          that a batch keeps its device address and content between those passes.  The first pass that scans a
 *                          slice then counts its k-mers for all n ranges in one histogram scan and keeps the count matrices (<= 4 GB);
 *                          the other passes skip that scan.  Results never depend on it.  Setting the option drops what is kept. */
/*   KQ_OPT_KERNEL_SET      measurement only (results never depend on it): bit mask of count-path stages that run their ALTERNATIVE kernel
 *                          instead of the shipped one, so that both can be timed in one process on the same buffers
 *                          (tools/bench_extra/alt_kernels.sh, bench.py --alt-kernels): 1 = P1 scatter of narrow and hash-remainder records with k_p1_scatter
 *                          (round 2's) instead of k_p1_scatter_s, 2 = split levels that write narrow records with k_lv_scatter_s (the
 *                          streamed formulation, which lost there) instead of k_lv_scatter, 4 = the level that writes tight records
 *                          with k_lv_scatter (round 2's) instead of k_lv_scatter_s, 16 = the table pass of 4- and 5-byte records with
 *                          k_count_regions_q4 (every wave reads its region's offsets from the sets' own offset arrays, through the
 *                          descriptors in memory, and the region's totals go to the table state with two atomics per region) instead of
 *                          k_p3_region_offsets + k_count_regions_q4r + k_fold_totals, 32 = the last split level of a plan with a middle
 *                          level through the unit path (k_lv_hist + offsets + scans + k_lv_scatter_s) also where the slice's even
 *                          buckets would select k_lv_segment_s (one workgroup per sub-bucket segment), 64 = k_lv_segment_s wherever
 *                          it applies, whatever the buckets look like and also in passes that do not read them back (tests,
 *                          measurement), 128 = the P1 scatter of narrow records behind a map-range filter with k_p1_scatter_s (every
 *                          k-mer hashed and parked, the dropped ones too) instead of k_p1_scatter_c (survivors queued per wave ahead of
 *                          the hash); bit 1 selects k_p1_scatter there too.  (8 is not assigned.)  Default 0. */
/*   KQ_OPT_SUBGRAPH_BATCH  (on the DATABASE handle) searches per batch of kq_subgraph_best_first; 0 (default) = automatic: a scratch arena of
 *                          1 GiB divided by the bytes of one search's state block at the call's depth.  Results never depend on it. */
/*   KQ_OPT_VARIANT_BATCH   searches per batch of kq_search_variants; 0 (default) = automatic: a scratch arena of 1 GiB divided by the
 *                          bytes of one search's state block at the call's depth and span.  Results never depend on it. */
enum { KQ_OPT_TRUST_CAPACITY = 1, KQ_OPT_COUNT_PATH = 2, KQ_OPT_SLICE_KMERS = 3, KQ_OPT_COUNT_MAP_RANGE = 4, KQ_OPT_PROFILE = 5,
       KQ_OPT_LOOKUP_PATH = 6, KQ_OPT_MERGE_PATH = 7, KQ_OPT_NARROW_MID = 8, KQ_OPT_PENDING_BYTES = 9, KQ_OPT_BUCKET_WINDOW = 10, KQ_OPT_OVERLAP = 11, KQ_OPT_COUNT_MAP_PASSES = 12, KQ_OPT_KERNEL_SET = 13, KQ_OPT_SHARD_WINDOW = 14, KQ_OPT_SUBGRAPH_BATCH = 15, KQ_OPT_VARIANT_BATCH = 16,
       KQ_OPT_TEST_FAIL_PLAN = 100 /* failure-path tests only: the next partition plan of a count fails with KQ_ERR_NOMEM */,
       KQ_OPT_TEST_EXPORT = 101 /* export-path tests only (results never depend on it; default 0): bit 0 = key order on the host, as when the device
                                   has no memory for the sort (kq_export; kq_export_map_images and kq_subgraph_gfa have no host sort and fail
                                   with KQ_ERR_NOMEM), bit 1 = results leave the device through the bounce buffers at any size, 4096 bytes a chunk */ };
int  kq_set_option(kq_handle* h, int option, int64_t value);
int  kq_get_profile(kq_handle* h, char* buf, uint64_t cap);
int  kq_sync(kq_handle* h);
/* Enqueue the table pass that applies all pending record sets (KQ_OPT_PENDING_BYTES); asynchronous, no-op when
 * nothing is pending.  kq_sync() and every call that reads the table do this themselves. */
int  kq_flush(kq_handle* h);
int  kq_get_info(kq_handle* h, kq_info* out);
const char* kq_last_error(void);
int  kq_abi_version(void);
/* 1 when a gfx950-capable device is visible to the HIP runtime. */
int  kq_device_available(void);
/* Free / total HBM of a device in bytes (what gfalibs' get_mem_total / freeMemory are to the reference's
 * memory-bounded mode, src/main.cpp:433, src/kreeq.cpp:59-63): lets the host choose how many map ranges to count in. */
int  kq_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes);

/* ---- hot loop 1 + 2: count ---------------------------------------------------------------- */

/* Replaces DBG::hashSequences (src/graph-builder.cpp:34-126) followed by DBG::processBuffers for
 * every map (:128-223) on one read batch: ASCII -> 2-bit, canonical key, edge byte, insert/RMW of
 * cov + 8 edge counters.  The key % mapCount disk partition of the reference has no counterpart
 * here (single table in HBM).  The host variant returns when the batch has been consumed; like the _dev variant it
 * may leave records pending (KQ_OPT_PENDING_BYTES): kq_sync() applies them and reports table-full conditions. */
int  kq_count_batch(kq_handle* h, const char* bases, uint64_t len);
int  kq_count_batch_dev(kq_handle* h, const char* d_bases, uint64_t len);

/* Pipelined host ingest (what gfalibs' loadKmers reader thread + readBatches queue are to the reference, src/input.cpp:95-96):
 * kq_count_batch_async enqueues the host-to-device copy of a batch on a copy stream and its count behind it, and returns
 * at once; copies overlap the counting of earlier batches (a small ring of device staging buffers).  `bases` should come
 * from kq_host_alloc (page-locked memory: the copy is a DMA at PCIe rate, 50+ GB/s here; a copy out of pageable memory the
 * runtime has not seen before costs ~1 ms per MiB for locking its pages) and be REUSED: a few buffers shared by all producer
 * threads beat a buffer per thread.  The buffer may be refilled once kq_host_wait(ticket)
 * has returned.  kq_count_batch_async may be called from several threads at once on one handle (the only entry point
 * that may; the calls take turns inside, none of them waits for the GPU); no other call on the handle may run concurrently
 * with them.  kq_sync() drains everything. */
/* kq_host_free: no copy may still read the buffer -- wait for the tickets of every batch submitted from it (kq_host_wait), or
 * kq_sync(), first; the library does not wait for them here. */
void* kq_host_alloc(uint64_t bytes);
void  kq_host_free(void* p);
int  kq_count_batch_async(kq_handle* h, const char* bases, uint64_t len, uint64_t* ticket);
int  kq_host_wait(kq_handle* h, uint64_t ticket);

/* 2-bit packed input (the "2-bit packing" step of the reference's kcount ancestry, moved in front of PCIe): kq_pack_bases
 * (host, no GPU) turns `len` bytes of bases + separators into ceil(len / 16) units of one u32 of 2-bit codes (base i of the
 * unit at bits 2i; A C G T = 0 1 2 3, case-blind) and one u16 of invalid-base bits (anything but ACGT/acgt -- read
 * separators, N -- and the positions behind `len` in the last unit).  That is the tile scanner's own format: 6 bytes per
 * 16 bases cross PCIe instead of 16, and the count kernels skip the ASCII conversion.  kq_count_packed_dev /
 * kq_count_packed_async count such a batch exactly like kq_count_batch_dev / kq_count_batch_async count its ASCII form
 * (same tickets, same threading rule; `codes` and `inv` may be refilled once kq_host_wait(ticket) has returned). */
void kq_pack_bases(const char* bases, uint64_t len, uint32_t* codes, uint16_t* inv);
int  kq_count_packed_dev(kq_handle* h, const uint32_t* d_codes, const uint16_t* d_inv, uint64_t n_bases);
int  kq_count_packed_async(kq_handle* h, const uint32_t* codes, const uint16_t* inv, uint64_t n_bases, uint64_t* ticket);

/* The same packing on the device: d_bases (ASCII, any alignment) -> d_codes / d_inv (ceil(len / 16) units each), bit-identical
 * to kq_pack_bases; asynchronous on the handle's stream.  This is how a caller makes the resident packed form of a batch that
 * kq_count_packed_dev counts (6 bytes per 16 bases of HBM instead of 16) without a host round trip. */
int  kq_pack_bases_dev(kq_handle* h, const char* d_bases, uint64_t len, uint32_t* d_codes, uint16_t* d_inv);

/* FASTQ / FASTA text on the device (what gfalibs' StreamObj line reader and loadKmers' record walk are to the reference,
 * src/input.cpp:188-286): the text goes to the GPU as it lies in the file and hand-written kernels find the bases.
 * `text` holds WHOLE RECORDS: it begins at the first byte of a record and ends at the end of one (a final '\n' is optional);
 * cutting a file at record starts stays with the caller.  Let l(i) be the number of '\n' before byte i (a '\n' belongs to the
 * line it ends) and EOL-CR a '\r' directly followed by '\n'.  The read batch is the kept bytes in text order:
 *   KQ_FASTX_FASTQ  four-line records: byte i is kept iff l(i) mod 4 == 1 and it is no EOL-CR.  The '\n' of a sequence line
 *                   is the read separator: seq0\nseq1\n...
 *   KQ_FASTX_FASTA  a line whose first byte is '>' is a header line: only its '\n' is kept (the separator).  Of any other line
 *                   every byte is kept except '\n' and EOL-CR, so wrapped sequence lines join: \nseq0\nseq1...
 * (One difference from the host CLI's parser: that one trims every trailing '\r' of a line, this one only the EOL-CR -- "\r\r\n"
 * inside a wrapped FASTA record ends the run here.)  Positions are 64-bit throughout: no size limit but the memory.
 * Malformed text is refused, not miscounted: a FASTQ line with l mod 4 == 0 that does not start with '@' or one with
 * l mod 4 == 2 that does not start with '+' (wrapped records ...), a FASTA text that does not start with '>'.
 *   kq_parse_fastx_dev   text -> d_bases (room for cap bytes), *n_bases = size of the batch.  Synchronises.  KQ_ERR_CAPACITY
 *                        (with *n_bases set) when cap is too small; d_bases may be NULL to get *n_bases only; KQ_ERR_INVALID
 *                        for malformed text (d_bases is unspecified then).
 *   kq_count_fastx_dev   parse into a library-owned buffer + count, like kq_count_batch_dev of the batch; nothing but the batch
 *                        size (one 16-byte read, which waits for the stream) returns to the host.
 *   kq_count_fastx_async text in page-locked host memory -> copy -> parse -> count: same tickets, same threading rule and the
 *                        same buffer reuse rule as kq_count_batch_async.  The call waits for its own copy and parse (on the
 *                        copy stream, beside the counting of earlier batches), not for any counting.
 * Malformed text given to the two count entries is not counted: kq_host_wait of its ticket and every kq_sync up to the next
 * kq_clear return KQ_ERR_INVALID with a message that names the format; the handle stays usable after kq_clear.
 * Null pointers or an unknown format: KQ_ERR_INVALID before any device work.  len == 0: KQ_OK, *n_bases = 0. */
enum { KQ_FASTX_FASTQ = 1, KQ_FASTX_FASTA = 2 };
int  kq_parse_fastx_dev(kq_handle* h, const char* d_text, uint64_t len, int format, char* d_bases, uint64_t cap, uint64_t* n_bases);
int  kq_count_fastx_dev(kq_handle* h, const char* d_text, uint64_t len, int format);
int  kq_count_fastx_async(kq_handle* h, const char* text, uint64_t len, int format, uint64_t* ticket);

/* BGZF-compressed reads (the block-gzip container of bgzip / htslib: valid multi-member gzip in which every member is an
 * independent DEFLATE stream of at most 64 KiB in and 64 KiB out, with its compressed size in the header's 'BC' extra subfield
 * and CRC-32 + ISIZE in the trailer).  The compressed bytes go to the GPU, one member per wave is inflated there, and the text
 * feeds the device parser above: no text touches the host.  Plain single-member gzip is not handled here.
 *   kq_bgzf_scan         host only, no device: walks members from data[0].  A member is accepted iff ID1 ID2 CM FLG = 1f 8b 08 04,
 *                        its extra field has a subfield 'B' 'C' of SLEN 2 (BSIZE), and with size = BSIZE + 1, data_off = 12 + XLEN,
 *                        data_len = size - XLEN - 20 >= 0 and ISIZE <= 65536.  It stops at the first member that does not lie wholly
 *                        inside len: *consumed = its offset, KQ_OK (feed a file piecewise).  A member that is not BGZF:
 *                        KQ_ERR_INVALID, *consumed = its offset, *n_blocks = the blocks before it (a plain .gz shows on the first
 *                        member).  More than cap blocks: KQ_ERR_CAPACITY, *n_blocks = the number needed.  Every read is checked
 *                        against len.
 *   kq_inflate_bgzf_dev  d_comp (device, comp_len bytes, any alignment) holds the members of `blocks` (a HOST array, `off` relative
 *                        to d_comp).  d_text receives the concatenation of their texts; *n_text = the sum of ISIZE.  Synchronises.
 *                        KQ_ERR_CAPACITY (with *n_text set) when cap is too small; d_text may be NULL to get *n_text only.
 *                        KQ_ERR_INVALID for a list that does not lie inside comp_len, and for a member that fails (invalid DEFLATE
 *                        data, a size other than ISIZE, a CRC-32 mismatch): the message names the FIRST failing member's index
 *                        and the reason.  A failing member writes nothing; bytes at and behind *n_text are never written.
 *                        n_blocks == 0: KQ_OK, *n_text = 0.
 *   kq_count_bgzf_dev    a STREAM on the handle: consecutive calls carry the pieces of one file, in file order.  The first call
 *                        begins at a record start.  Each call inflates its members behind the carry the previous call left on
 *                        the device, finds the end of the last whole record (FASTQ: the byte after the last '\n' whose ordinal
 *                        from the start of the text is a multiple of 4; FASTA: the last '>' that starts a line, if it is not the
 *                        text's first byte), counts the text in front of it exactly as kq_count_fastx_dev counts that text, and
 *                        keeps the rest as the new carry.  With KQ_BGZF_END the whole remaining text is counted (a final '\n'
 *                        is optional) and the stream is empty again; kq_clear empties it too.  n_blocks == 0 is allowed.  Two
 *                        small read-backs per call, each of which waits for the stream: the status record (failed member, cut),
 *                        then the parser's batch size.
 * The three device entries share staging buffers of the handle: one caller at a time per handle, like every entry point that
 * works on the handle's stream.  (Compressed bytes in page-locked HOST memory have no entry of their own yet: copy them with
 * kq_copy_async into a kq_dev_alloc block and call kq_count_bgzf_dev.)
 * A corrupt member, or text the parser refuses, is not counted: every kq_sync up to the next kq_clear returns KQ_ERR_INVALID (for
 * a corrupt member with its index in the call and the reason); a corrupt member also drops the carry.  Null pointers, an unknown
 * format or flag, a block list outside comp_len: KQ_ERR_INVALID before any device work. */
typedef struct { uint64_t off; uint32_t size; uint32_t data_off; uint32_t data_len; uint32_t crc32; uint32_t isize; } kq_bgzf_block;
enum { KQ_BGZF_END = 1 };
int  kq_bgzf_scan(const void* data, uint64_t len, kq_bgzf_block* blocks, uint64_t cap, uint64_t* n_blocks, uint64_t* consumed);
int  kq_inflate_bgzf_dev(kq_handle* h, const void* d_comp, uint64_t comp_len, const kq_bgzf_block* blocks, uint64_t n_blocks,
                         char* d_text, uint64_t cap, uint64_t* n_text);
int  kq_count_bgzf_dev(kq_handle* h, const void* d_comp, uint64_t comp_len, const kq_bgzf_block* blocks, uint64_t n_blocks, int format, uint32_t flags);

/* Text -> BGZF, the other direction: the text is cut into members of 0xff00 bytes (bgzip's choice; the last one shorter), every
 * member is compressed by one wave on the GPU (LZ77 with a hash table in LDS, one dynamic-Huffman block, or one stored block when
 * that is not smaller: no member is larger than 18 + 5 + its text + 8 bytes), and the members lie back to back in the output.
 * The bytes are a function of the text alone: not of the alignment of d_text, the launch geometry or the schedule.
 *   kq_bgzf_bound        host only: the largest output kq_deflate_bgzf_dev can produce for n_text bytes with these flags
 *                        (n_text + 31 per member, + 28 with KQ_BGZF_EOF).
 *   kq_deflate_bgzf_dev  d_text (device, any alignment) -> d_out (device, any alignment, room for cap bytes); *n_out = the bytes
 *                        written.  KQ_BGZF_EOF appends the standard 28-byte empty member that ends a BGZF file.  cap below
 *                        kq_bgzf_bound: KQ_ERR_CAPACITY with *n_out = the bound, before any device work.  n_text == 0 writes
 *                        nothing, or only the marker.  The outputs of successive calls, concatenated, are one valid BGZF file.
 *                        Runs on the handle's stream and synchronises; one caller at a time, like the entries above.
 *   kq_deflate_bgzf      the same from and to HOST buffers (staging, the device call, the copy back): tests and small callers.
 * Null pointers (h, n_out; d_text with n_text, d_out with cap) or unknown flag bits: KQ_ERR_INVALID before any device work. */
enum { KQ_BGZF_EOF = 2 };
uint64_t kq_bgzf_bound(uint64_t n_text, uint32_t flags);
int  kq_deflate_bgzf_dev(kq_handle* h, const char* d_text, uint64_t n_text, void* d_out, uint64_t cap, uint64_t* n_out, uint32_t flags);
int  kq_deflate_bgzf(kq_handle* h, const char* text, uint64_t n_text, void* out, uint64_t cap, uint64_t* n_out, uint32_t flags);

/* Hot loop 1 only (DBG::hashSequences :75-113): the (key, edge byte) records of a batch in
 * sequence order; edge byte layout = edgeBit (include/kreeq.h:6-18).  *n_out = number of records
 * (also set on KQ_ERR_CAPACITY).  keys/edges may be NULL to just count. */
int  kq_emit_records(kq_handle* h, const char* bases, uint64_t len,
                     uint64_t* keys, uint8_t* edges, uint64_t cap, uint64_t* n_out);
/* Device variant used to stage the multi-GPU exchange: records are grouped by owner part
 * (part p owns the maps m with floor(m * n_parts / map_count) == p, m = key % map_count; order
 * inside a part is unspecified).  d_keys/d_edges need room for len records; part_counts[n_parts]
 * is a HOST array. Synchronises. */
int  kq_emit_partitioned_dev(kq_handle* h, const char* d_bases, uint64_t len, int n_parts,
                             uint64_t* d_keys, uint8_t* d_edges, uint64_t cap,
                             uint64_t* part_counts);

/* Same staging with PACKED 8-byte records (k <= 28): bits 0..55 = the library's invertible 56-bit mix
 * of the canonical key (its table hash; opaque to the caller, identical on every handle with the same
 * k), bits 56..58 / 59..61 = index of the fw / bw edge the instance contributes (0..3, 7 = none;
 * src/graph-builder.cpp:98-110).  One array to exchange instead of two, and the receive side
 * (kq_insert_packed_dev, the only consumer of this format) runs the partitioned, atomic-free count
 * without hashing again.  d_recs needs room for len - k + 1 records.  Synchronises. */
int  kq_emit_packed_dev(kq_handle* h, const char* d_bases, uint64_t len, int n_parts,
                        uint64_t* d_recs, uint64_t cap, uint64_t* part_counts);
int  kq_insert_packed_dev(kq_handle* h, const uint64_t* d_recs, uint64_t n);

/* Multi-GPU staging with 5-BYTE records (k <= 21, the default k): d_recs[i] (u32) + d_aux[i] (u8) = the hash bits below
 * the 8-bit hash-prefix bucket of record i and its two edge indices -- the record format of the single-GPU count, written
 * by its first (bucket) split.  OWNERSHIP IS BY BUCKET RANGE: part p of n_parts owns the buckets
 * [ceil(256 p / n_parts), ceil(256 (p + 1) / n_parts)), so the bucket-sorted output is already grouped by owner: the part
 * of every owner is one contiguous run (part_counts, host), and d_bucket_counts[p * 256 + b] (DEVICE, n_parts x 256) =
 * records of bucket b if p owns it, else 0.  The receiver gets, from every peer, its run and that peer's 256 counts for it
 * (one all-to-all(v) per array + one all-to-all of 256 counts) and calls kq_insert_sharded_dev with the runs concatenated
 * in peer order and d_bucket_counts = [n_peers x 256] (DEVICE, peer-major): the records enter the bucket -> region split
 * levels directly.  The receiving handle is the window of its buckets (KQ_OPT_BUCKET_WINDOW; with one part: an ordinary
 * table) and must have >= 2048 regions; records of buckets outside its window are ignored.
 * (The reference's key % mapCount -- src/graph-builder.cpp:95 -- remains the layout of the database FILES: export filters
 * by map range on every shard.)  Buffers need room for len - k + 1 records.  kq_emit_sharded_dev synchronises to fill
 * part_counts; with part_counts == NULL it only enqueues (the part sizes are the row sums of d_bucket_counts: a caller that
 * exchanges the counts anyway reads them in the same host round trip). */
int  kq_emit_sharded_dev(kq_handle* h, const char* d_bases, uint64_t len, int n_parts, uint32_t* d_recs, uint8_t* d_aux, uint64_t cap,
                         uint64_t* d_bucket_counts, uint64_t* part_counts);
int  kq_insert_sharded_dev(kq_handle* h, const uint32_t* d_recs, const uint8_t* d_aux, uint64_t n, int n_peers, const uint64_t* d_bucket_counts);

/* The same staging for k = 29..32 with 8-BYTE HASH-REMAINDER records: d_recs[i] (u64) = bits 8..63: the 56 bits of the k-mer's
 * table hash below its 8-bit hash-prefix bucket, bits 0..5: its two edge indices, bits 6..7: zero -- the record format of the
 * single-GPU count at these k, written by its first (bucket) split; opaque to the caller and stable within an ABI version
 * like the other record formats.  A record and the bucket of the run it lies in are the whole k-mer.  Everything else is the
 * contract of kq_emit_sharded_dev / kq_insert_sharded_dev with one array instead of two: parts are the bucket ranges
 * [ceil(256 p / n_parts), ceil(256 (p + 1) / n_parts)), the output is bucket-sorted (every part one run), d_bucket_counts is
 * [n_parts x 256] on the DEVICE, part_counts == NULL only enqueues; the sending handle needs no particular table (a window
 * it may have is not applied: every bucket is emitted).  KQ_ERR_INVALID for k outside 29..32, n_parts outside 1..256 or null
 * pointers, KQ_ERR_CAPACITY when cap < len - k + 1, fewer than 2^32 k-mer starts per call; len < k: all counts zero, KQ_OK.
 * kq_insert_sharded8_dev takes the runs of all peers concatenated in peer order and d_bucket_counts = [n_peers x 256]
 * (DEVICE, peer-major); the receiving handle is the window of its buckets (KQ_OPT_SHARD_WINDOW; with one part: an ordinary
 * table) and must have >= 2048 regions (KQ_ERR_INVALID otherwise: smaller tables take kq_emit_partitioned_dev /
 * kq_insert_records_dev); records of buckets outside its window are ignored.  Pending sets (KQ_OPT_PENDING_BYTES) and table
 * growth work as for a count.  8 bytes per record in one all-to-all(v) instead of 9 in two. */
int  kq_emit_sharded8_dev(kq_handle* h, const char* d_bases, uint64_t len, int n_parts, uint64_t* d_recs, uint64_t cap,
                          uint64_t* d_bucket_counts, uint64_t* part_counts);
int  kq_insert_sharded8_dev(kq_handle* h, const uint64_t* d_recs, uint64_t n, int n_peers, const uint64_t* d_bucket_counts);

/* Hot loop 2 only (DBG::processBuffers :160-206) on explicit records. */
int  kq_insert_records(kq_handle* h, const uint64_t* keys, const uint8_t* edges, uint64_t n);
int  kq_insert_records_dev(kq_handle* h, const uint64_t* d_keys, const uint8_t* d_edges, uint64_t n);

/* ---- summary ------------------------------------------------------------------------------ */

/* Replaces DBG::summary(m) for all m + DBG::DBstats (src/graph-builder.cpp:240-295). */
int  kq_summary(kq_handle* h, kq_stats* out);
/* finalHistogram (src/graph-builder.cpp:274-278; printed by gfalibs printHist): (cov, count)
 * pairs sorted by cov.  cov/cnt may be NULL to get *n_out only. */
int  kq_histogram(kq_handle* h, uint64_t* cov, uint64_t* cnt, uint64_t cap, uint64_t* n_out);

/* ---- hot loop 3: assembly lookup + QV counters --------------------------------------------- */

/* Replaces DBG::evaluateSegment (src/kreeq.cpp:110-229) for every segment of one assembly
 * sequence: the sequence is split into segments at non-ACGT bytes; every k-mer whose map index
 * key % map_count lies in [map_lo, map_hi) is looked up.  counters[0] += missing,
 * counters[1] += k-mers evaluated, counters[2] += edge-missing (the three atomics of
 * include/kreeq.h:152).  per_base (nullable) has `len` entries aligned with `bases`, must be
 * zero-initialised by the caller before the first map range (generateValidationVector,
 * src/input.cpp:38-45) and is updated only at evaluated positions. */
int  kq_lookup_sequence(kq_handle* h, const char* bases, uint64_t len, uint32_t cov_cutoff,
                        uint16_t map_lo, uint16_t map_hi, kq_dbgbase* per_base,
                        uint64_t counters[3]);
/* d_counters: 3 x u64 on the device, accumulated with atomics (zero them first). Asynchronous. */
int  kq_lookup_sequence_dev(kq_handle* h, const char* d_bases, uint64_t len, uint32_t cov_cutoff,
                            uint16_t map_lo, uint16_t map_hi, kq_dbgbase* d_per_base,
                            uint64_t* d_counters);

/* ---- per-base tables (.kwig / .bkwig / .bed / .csvtable; src/kreeq-output.cpp:138-399, src/decompressor.cpp:493-585) ------ */

/* Device memory for callers that do not link the HIP runtime (the CLI): a block on the handle's GPU, zero-filled on the
 * handle's stream, owned by the handle (kq_destroy frees what kq_dev_free has not; NULL when there is no memory).
 * kq_dev_free waits for the device.  kq_copy_async: dst <- src, `bytes` bytes,
 * asynchronous on the handle's stream (host memory should come from kq_host_alloc); kq_sync() waits for it. */
enum { KQ_COPY_TO_DEVICE = 1, KQ_COPY_TO_HOST = 2 };
void* kq_dev_alloc(kq_handle* h, uint64_t bytes);
void  kq_dev_free(kq_handle* h, void* p);
int   kq_copy_async(kq_handle* h, void* dst, const void* src, uint64_t bytes, int kind);

/* The payload of a .bkwig from the per-base array of a lookup (src/kreeq-output.cpp:357-399): the entries of the listed
 * segments (seg_start[s] = index of the segment's first entry in d_per_base, seg_len[s] entries; host arrays), in order, as
 * ORIENTED u32 triples: cov, isFw ? fw : bw, isFw ? bw : fw.  d_triples receives sum(seg_len) x 12 bytes; what lies between
 * the segments (separators, N runs) is dropped.  The kernel is enqueued on the handle's stream and the call does not wait
 * for it; it does wait for what the stream held before (the segment lists are copied first).  KQ_ERR_INVALID for null
 * pointers or 2^32 - 1 segments and more; no segment or only empty ones: KQ_OK without device work. */
int  kq_per_base_triples_dev(kq_handle* h, const kq_dbgbase* d_per_base, const uint64_t* seg_start, const uint64_t* seg_len,
                             uint64_t n_segs, uint32_t* d_triples);

/* The same payload accumulated over map-range passes.  The lists mean what they mean above (position g of the output is
 * entry seg_start[s] + g - (positions of the segments before s)), and per listed position: an entry with any of its 16 bytes
 * non-zero is STORED -- its oriented triple is written to d_triples[3g .. 3g + 2] and the entry is set to 16 zero bytes; an
 * all-zero entry leaves its triple untouched.  Nothing between the segments is read or written.  Afterwards d_per_base is
 * zero over the listed segments again, so the same array serves the next lookup (the next group of sequences or the next
 * map range) without a memset, and because a position is evaluated in exactly one map range and a lookup stores only found
 * k-mers, d_triples (zeroed once) holds after all ranges what kq_per_base_triples_dev gives after one whole-range lookup.
 * Asynchronous like kq_per_base_triples_dev; KQ_ERR_INVALID also for segments that are not ascending and non-overlapping
 * (seg_start[s] >= seg_start[s - 1] + seg_len[s - 1]; checked on the host before any device work). */
int  kq_per_base_merge_dev(kq_handle* h, kq_dbgbase* d_per_base, const uint64_t* seg_start, const uint64_t* seg_len,
                           uint64_t n_segs, uint32_t* d_triples);

/* Triples -> decimal text, formatted on the device.  A call formats PIECES in order; piece p covers the triples
 * first .. first + n - 1 and the coordinates abs_pos .. abs_pos + n - 1, and names + name_off / name_len is its sequence name.
 *   KQ_TABLE_KWIG  per piece: when flags has KQ_TABLE_SEG_HEADER the line "fixedStep chrom=<name> start=<abs_pos> step=1\n",
 *                  then "c,f,b\n" per position (src/kreeq-output.cpp:275-281)
 *   KQ_TABLE_BED   column separator '\t', entry separator ':'        KQ_TABLE_CSV   both ','
 *                  the line of position i is <name><col><abs_pos + i><col>W(cov)<col>W(fw)<col>W(bw)\n, W(x) = the k values
 *                  of column x at positions i - k + 1 .. i, oldest first, joined by the entry separator; k = the handle's k
 *                  (src/kreeq-output.cpp:176-219, src/decompressor.cpp:534-579).  The n_ctx triples before `first` are the
 *                  window's history (a segment cut into pieces: n_ctx = min(cut, k - 1)); a position before that reads as 0.
 *                  A window never reads across a piece boundary beyond n_ctx.  (KQ_TABLE_KWIG ignores n_ctx beyond checking it.)
 * The output is the concatenated text.  *n_out = its size, always set on KQ_OK and KQ_ERR_CAPACITY.  out == NULL: the size
 * query.  cap < size: KQ_ERR_CAPACITY, nothing is written.  Offsets are 64-bit; a call takes fewer than 2^32 lines.
 * KQ_ERR_INVALID before any device work: null pointers (h, n_out; segs with n_segs, triples with n_triples, names with
 * names_len), an unknown format, n_ctx > k - 1 or n_ctx > first, first + n > n_triples, a name outside `names` or longer than
 * 65535 bytes, 2^32 lines or more.  No piece or no line: KQ_OK, *n_out = 0.  The bytes do not depend on the launch geometry,
 * and cutting a segment into pieces (the first with the header flag, the others with their n_ctx) gives the bytes of the
 * whole segment.  kq_format_table_dev takes device `d_triples` / `d_out`, kq_format_table host memory; `segs` and `names` are
 * host memory in both.  Both synchronise. */
typedef struct { uint64_t first, n, abs_pos; uint32_t name_off, name_len, n_ctx, flags; } kq_table_seg;      /* 40 bytes */
enum { KQ_TABLE_SEG_HEADER = 1 };
enum { KQ_TABLE_KWIG = 1, KQ_TABLE_BED = 2, KQ_TABLE_CSV = 3 };
int  kq_format_table_dev(kq_handle* h, int format, const uint32_t* d_triples, uint64_t n_triples, const kq_table_seg* segs, uint64_t n_segs,
                         const char* names, uint64_t names_len, char* d_out, uint64_t cap, uint64_t* n_out);
int  kq_format_table(kq_handle* h, int format, const uint32_t* triples, uint64_t n_triples, const kq_table_seg* segs, uint64_t n_segs,
                     const char* names, uint64_t names_len, char* out, uint64_t cap, uint64_t* n_out);

/* ---- candidate-error search support (DBG::correctSequences, src/variants.cpp) --------------------------------- */

/* Batched map->find(key) (src/variants.cpp:118-131, :203-206; src/kreeq.cpp:152-166 for the 32-bit tier): the logical
 * entries of n canonical keys, out[i].key = keys[i]; out[i].cov == 0 when the k-mer is absent.  The bounded graph
 * search stays on the host (pointer chasing, serial per source); it asks for its frontier in batches through this. */
int  kq_lookup_keys(kq_handle* h, const uint64_t* keys, uint64_t n, kq_entry* out);

/* Device pre-filter of the search: for every k-mer start c of `bases` (segments = ACGT runs, like kq_lookup_sequence),
 * flags[c] bit 0 = the k-mer is in the table, bit 1 = DBG::searchVariants would find at least one candidate path at
 * its source (src/variants.cpp:232-246 at depth 0): an edge in the direction the sequence is read, with a count
 * above cov_cutoff, that does not lead to the k-mer the sequence continues with.  Only those positions need the host
 * search; everywhere else it returns at once without a variant.  flags has `len` bytes (0 where no k-mer starts). */
int  kq_branch_scan(kq_handle* h, const char* bases, uint64_t len, uint32_t cov_cutoff, uint8_t* flags);

/* The whole candidate-error search on the device (DBG::DBGtoVariants + searchVariants, src/variants.cpp:53-310, single map
 * range): the pre-filter of kq_branch_scan, then one bounded graph search per flagged position -- one search per lane on a
 * fixed-size state block (csrc/kq_variant_core.h), in batches of KQ_OPT_VARIANT_BATCH -- and the paths of all of them.
 *   bases      what kq_branch_scan takes: host memory, segments = ACGT runs, len < 2^32 - 1
 *   depth      --search-depth, 0 .. 253; max_span: --max-span, 0 .. 255 (the device limits; why 253: kq_variant_core.h).
 *              max_span 0: the reference pops an empty queue; read as "the pop is skipped", the one target is k-mer c + k.
 *   paths      one record per path, in ascending pos and, within one position, in destination order (the order of the
 *              reference's `destinations`): pos = index in `bases` of the first base behind the source k-mer (c + k),
 *              seg_start = index of the first base of that position's segment, seq + seq_off / seq_len = the path's bases
 *              in upper case (not terminated), type = KQ_VAR_*, ref_len != 0 for KQ_VAR_COM only.
 *   *n_paths, *n_seq   records and sequence bytes of the whole result; always set on KQ_OK and KQ_ERR_CAPACITY.
 * paths == NULL or seq == NULL: only the two counts.  path_cap (records) or seq_cap (bytes) too small: KQ_ERR_CAPACITY with
 * both counts set and nothing written; the searches are NOT kept, a repeat with larger buffers runs them again.  Null
 * n_paths / n_seq, a windowed handle (KQ_OPT_BUCKET_WINDOW / KQ_OPT_SHARD_WINDOW), depth or max_span outside the limits, or
 * len >= 2^32 - 1: KQ_ERR_INVALID before any device work.  len < k: KQ_OK, both counts zero.  Flushes pending records and
 * synchronises.  Results do not depend on the batch size or on the launch geometry. */
typedef struct { uint64_t pos, seg_start, seq_off; uint16_t seq_len, ref_len; uint8_t type, pad[3]; } kq_variant_path; /* 32 bytes */
enum { KQ_VAR_SNV = 0, KQ_VAR_INS = 1, KQ_VAR_DEL = 2, KQ_VAR_COM = 3 };
int  kq_search_variants(kq_handle* h, const char* bases, uint64_t len, int depth, int max_span, uint32_t cov_cutoff,
                        kq_variant_path* paths, uint64_t path_cap, uint64_t* n_paths,
                        char* seq, uint64_t seq_cap, uint64_t* n_seq);

/* ---- union / database import-export --------------------------------------------------------- */

/* Replaces DBG::kunion + DBG::mergeSubMaps (src/graph-builder.cpp:297-432): dst += src, exact
 * saturating sums; both handles must live on the same device. */
int  kq_merge(kq_handle* dst, kq_handle* src);

/* Replaces phmap_load of <db>/.map.<m>.bin + .map.hc.bin (src/graph-builder.cpp:307-308, gfalibs
 * loadMapRange): ADDS logical entries to the table (importing two databases == union). */
int  kq_import(kq_handle* h, const kq_entry* entries, uint64_t n);
/* Replaces gfalibs dumpMap/dumpHighCopyKmers: logical entries with key % map_count in
 * [map_lo, map_hi), sorted by key.  out may be NULL to get *n_out only. */
int  kq_export(kq_handle* h, uint16_t map_lo, uint16_t map_hi, kq_entry* out, uint64_t cap,
               uint64_t* n_out);


/* Replaces gfalibs dumpMap (and the host writer's insertion emulation): the complete bytes of <db>/.map.<m>.bin for every
 * map m in [map_lo, map_hi), built on the device.  out + offsets[m - map_lo] .. out + offsets[m - map_lo + 1] is the file
 * of map m (offsets: map_hi - map_lo + 1 values, host): the phmap dump of 256 submaps that sequential insertion in
 * ascending unsigned key order gives, byte for byte what the host writer produces from kq_export's entries of the range.
 * A high-copy k-mer (hc != 0) becomes the tombstone slot (cov 255, edges 0); those entries are returned in hc_out, sorted
 * by key, for the single .map.hc.bin the host writes.  out == NULL: only offsets and *n_hc are filled (the size query: one
 * pass over the table).  KQ_ERR_CAPACITY, with offsets and *n_hc set, when cap (bytes) or hc_cap (entries) is too small;
 * KQ_ERR_INVALID for a bad range or null offsets / n_hc, before any device work, and for a range of 2^32 k-mers or more
 * (take smaller ranges).  The image, the range's entries and the sort scratch must fit beside the table: choose ranges
 * with the size query.  Flushes pending records; on a windowed handle the window's k-mers are exported.  Synchronises. */
int  kq_export_map_images(kq_handle* h, uint16_t map_lo, uint16_t map_hi, void* out, uint64_t cap, uint64_t* offsets,
                          kq_entry* hc_out, uint64_t hc_cap, uint64_t* n_hc);
/* Replaces phmap_load of one <db>/.map.<m>.bin (gfalibs loadMapRange): `image` (host memory, page-locked or not) holds the
 * whole file.  The 256 submap headers are walked and bound-checked on the host, the bytes go to the device as they are, one
 * kernel checks every occupied slot (occupied count == size, key % map_count == map, cov > 0, no edge counter above cov)
 * and a second one ADDS every slot with cov != 255 to the table (importing two databases == union).  Slots with cov == 255
 * are tombstones: counted in *n_tombstones and skipped -- their counters are in .map.hc.bin, which the caller imports with
 * kq_import and compares against the tombstone count.  A malformed image (submap count, version, truncated, trailing
 * bytes, size mismatch, wrong map, invalid entry) is refused with KQ_ERR_INVALID and nothing is added; the header defects
 * are found before any device work.  An empty map (6152 bytes) is KQ_OK without device work.  Synchronises. */
int  kq_import_map_image(kq_handle* h, uint16_t map, const void* image, uint64_t n_bytes, uint64_t* n_entries,
                         uint64_t* n_tombstones);

/* ---- subgraph (DBG::subgraph, traversal, removeMissingEdges, summary; src/subgraph.cpp) -------------------------------- */

/* The subgraph is a SECOND, ordinary handle `sub` with the k, map_count and device of the database handle `db`: kq_export,
 * kq_summary (the "Subgraph summary statistics" block, src/subgraph.cpp:163-188), kq_lookup_keys and kq_histogram read it
 * like any table.  Every call flushes the pending records of both handles first and synchronises.  KQ_ERR_INVALID, before
 * any device work, for null pointers, db == sub, a windowed handle (KQ_OPT_BUCKET_WINDOW / KQ_OPT_SHARD_WINDOW), unknown
 * flag bits and a depth outside 0..255; KQ_ERR_MISMATCH for handles that differ in k / map_count / device; the handles
 * stay usable after a refusal.
 *
 * kq_subgraph_seed(_dev)  Replaces DBGsubgraphFromSegment for every segment of the batch + mergeSubgraphs (:190-288, :42-112).
 *     The batch is cut into segments (ACGT runs) like kq_lookup_sequence cuts it.  Within ONE segment every canonical key counts
 *     once, and its first position decides: a key of the database adds its logical entry (exact 32-bit counters of either
 *     tier); an absent key adds, unless flags has KQ_SUBGRAPH_NO_REFERENCE, a constructed k-mer with cov 1 and the at most
 *     two edges its neighbours inside the segment at that position give (the edge rule of a count).  Segments ADD UP (a key of
 *     m segments holds m times its counters, saturating at 2^32 - 1), and so do calls: seeding two batches == seeding their
 *     concatenation with a separator.  The result does not depend on the launch geometry.  Batches below 2^32 - 1 bytes;
 *     device scratch: 25 to 33 bytes per base of the batch, freed before the call returns.  The _dev variant takes a device pointer valid on the handles' GPU.
 * kq_subgraph_expand      Replaces DBG::traversal (:301-415) for one resident map range: `depth` rounds; round 1 starts from the
 *     k-mers of `sub`, round r + 1 from those round r found; every edge counter != 0 of a frontier k-mer gives a neighbour
 *     (DBG::buildNextKmer, :581-597), which is found when it is not in `sub` and is in `db`.  What was found is inserted, with
 *     its database entry, after the last round.  The frontier stays on the device; its size returns to the host once per
 *     round, and an empty one ends the rounds.  *n_added = k-mers inserted.  KQ_ERR_TABLE_FULL when the frontier list, the
 *     visited set or `sub` cannot grow.
 * kq_subgraph_best_first  Replaces DBG::bestFirst / dijkstra (:417-579) for one resident map range: one search per k-mer of `sub`, at
 *     most depth + 1 pops each, all of a batch in ONE kernel launch with one search per lane (kq_bestfirst_core.h: a bounded
 *     state block of 9 + 4 depth nodes per search, KQ_OPT_SUBGRAPH_BATCH searches per batch).  Membership is tested against the
 *     seed set only; an edge counter > cov_cutoff is followed when its neighbour is in `db`; the source's counters are those of
 *     its `sub` entry, every other k-mer's its logical `db` entry.  The k-mers on the paths back from every destination are
 *     inserted, with their database entries, after the last batch.  Only a batch's total returns to the host.  *n_added =
 *     k-mers inserted; the result does not depend on the batch size or the launch geometry.  KQ_ERR_TABLE_FULL when the found
 *     list, the visited set or `sub` cannot grow; KQ_ERR_NOMEM when the state blocks of a batch cannot be allocated.
 * kq_subgraph_trim        Replaces DBG::removeMissingEdges (:599-625): every edge counter > cov_cutoff of `sub` whose neighbour
 *     k-mer is not in `sub` becomes 0, in both tiers; counters <= cov_cutoff are not examined.  Not to be mixed with inserts. */
enum { KQ_SUBGRAPH_NO_REFERENCE = 1 };
int  kq_subgraph_seed(kq_handle* db, kq_handle* sub, const char* bases, uint64_t len, uint32_t flags);
int  kq_subgraph_seed_dev(kq_handle* db, kq_handle* sub, const char* d_bases, uint64_t len, uint32_t flags);
int  kq_subgraph_expand(kq_handle* db, kq_handle* sub, int depth, uint64_t* n_added);
int  kq_subgraph_best_first(kq_handle* db, kq_handle* sub, int depth, uint32_t cov_cutoff, uint64_t* n_added);
int  kq_subgraph_trim(kq_handle* sub, uint32_t cov_cutoff);

/* kq_subgraph_gfa  The trimmed subgraph `sub` as the graph the reference hands to its GFA writer (DBG::DBGgraphToGFA and
 * DBG::collapseNodes, src/kreeq.cpp:360-600), built on the device.  An oriented k-mer is (key, +) = the canonical string or
 * (key, -) = its reverse complement; its id is 2 * rank of the key in ascending key order + (orientation == '-'); the
 * out-edges of (x,+) are the non-zero fw counters, those of (x,-) the non-zero bw counters.
 *   default          Non-branching runs become one segment each.  v -> w is a LINK when v has exactly one out-edge, w's key is
 *       in `sub` and is another key, neither key is its own reverse complement, and flip(w) has exactly one out-edge, which
 *       leads to flip(v).  Links form chains; a cycle is cut in front of its smallest oriented id; of a chain and its mirror
 *       the one whose head has the smaller id is kept and is a segment.  Segments are numbered by ascending head id; the
 *       sequence is the head's oriented k-mer plus the last base of every following one; cov is the head's.  Every other
 *       non-zero counter whose neighbour is in `sub` is an edge: emitted when the neighbour is the first k-mer of its chain
 *       (else counted in n_dropped_edges: asymmetric counters that point into a segment), once per bidirected pair (of an
 *       edge and its mirror the one with the smaller (source id, target id)), in ascending (source id, base) order.  An end's
 *       rc is 0 when the oriented k-mer lies on the kept chain.  A cycle is one segment with an edge from its + end to its + start.
 *   KQ_GFA_NO_COLLAPSE   Every k-mer is a segment (+, numbered by ascending key); per k-mer its fw lines `this + -> next`, then
 *       its bw lines `prev -> this +` (:545-594), nothing deduplicated; counters whose neighbour is absent give no line.
 * The reference numbers nodes, picks the cov and orders links by the iteration order of its hash map; the numbering, cov and
 * order here are this library's own.
 *   segs[i]   seq + seq_off: n_kmers + k - 1 bases (no terminator); head_key / head_rc: the first oriented k-mer; cov: its cov
 *   edges[j]  from (from_rc ? - : +) -> to (to_rc ? - : +), overlap k - 1, count = the counter that gave the edge
 *   counts    always set on KQ_OK and KQ_ERR_CAPACITY; n_cycles = segments that were cycles
 * segs, seq or edges NULL: only the counts.  A cap (records, bytes, records) too small: KQ_ERR_CAPACITY, nothing is written.
 * KQ_ERR_INVALID for a null sub / counts, unknown flag bits, a windowed handle, and 2^31 or more k-mers.  An empty table:
 * KQ_OK, all counts zero.  Flushes pending records and synchronises; device scratch (about 400 bytes per k-mer) is freed before
 * the call returns.  The result does not depend on the launch geometry. */
typedef struct { uint64_t seq_off, head_key; uint32_t n_kmers, cov; uint8_t head_rc, pad[7]; } kq_gfa_segment;      /* 32 bytes */
typedef struct { uint32_t from, to, count; uint8_t from_rc, to_rc, pad[2]; } kq_gfa_edge;                           /* 16 bytes */
typedef struct { uint64_t n_segments, n_seq, n_edges, n_dropped_edges, n_cycles; } kq_gfa_counts;
enum { KQ_GFA_NO_COLLAPSE = 1 };
int  kq_subgraph_gfa(kq_handle* sub, uint32_t flags, kq_gfa_segment* segs, uint64_t seg_cap, char* seq, uint64_t seq_cap,
                     kq_gfa_edge* edges, uint64_t edge_cap, kq_gfa_counts* counts);

#ifdef __cplusplus
}
#endif
#endif /* KREEQ_AMD_H */
