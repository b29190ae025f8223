/*
 * flowagg.h - C-ABI of libflowagg: the MI355X (gfx950) flow-aggregation stage.
 *
 * The reference (cloudflare/flow-pipeline) has no plugin/FFI interface; this ABI
 * is what a Go Kafka consumer binds through cgo to replace the
 * ClickHouse path `flows -> flows_raw -> flows_5m`
 * (compose/clickhouse/create.sh:5-110) while keeping the inserter's shape
 * (inserter/inserter.go:113-196: buffer -> flush -> sink).
 *
 * Conventions
 *  - plain C, no torch / HIP types in signatures; device pointers travel as
 *    `const void*` / `void*` and are documented as such;
 *  - every function returns 0 (FA_OK) or a negative fa_status; text via
 *    fa_last_error();
 *  - the library never keeps a caller pointer after a call returns (cgo rule):
 *    fa_ingest copies into library-owned pinned staging before returning;
 *  - one fa_ctx per (Kafka partition, GPU).  A ctx is not thread-safe; distinct
 *    ctxs are independent (sarama runs one ConsumeClaim goroutine per claimed
 *    partition, inserter.go:176);
 *  - malformed records are counted and dropped, never fatal
 *    (inserter.go:125-126); sink/resource errors are returned (the reference
 *    log.Fatal()s on them, inserter.go:102-105);
 *  - there is NO CPU fallback: without a HIP device fa_create fails.
 */
#ifndef FLOWAGG_H
#define FLOWAGG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_ABI_VERSION 8

typedef struct fa_ctx fa_ctx;

typedef enum {
    FA_OK = 0,
    FA_ERR_ARG = -1,        /* bad argument */
    FA_ERR_NO_DEVICE = -2,  /* no HIP device / HIP runtime error at create */
    FA_ERR_HIP = -3,        /* HIP runtime error (text in fa_last_error) */
    FA_ERR_NOMEM = -4,
    FA_ERR_TABLE_FULL = -5, /* a table cannot grow further (2^30 slots) or the distinct-address set behind fa_topk is
                               full.  Aggregates are never dropped on the way there: updates that meet a full table
                               are parked (the spill buffers hold everything the host may have in flight: 2 x
                               max_batch_records per table) and replayed after the table has grown - the host looks
                               at the device counters before every launch. */
    FA_ERR_CAPACITY = -6,   /* caller's output buffer too small; *n_out = required */
    FA_ERR_FRAMING = -7,    /* offsets==NULL and the stream is not a chain of framed records */
    FA_ERR_UNSUPPORTED = -8
} fa_status;

/* key_sets bitmask */
enum {
    FA_KEYS_AS_PAIR = 1u,     /* flows_5m: (Date,Timeslot,SrcAS,DstAS,EType) - create.sh:92-110 */
    FA_KEYS_SRCADDR_CMS = 2u, /* Count-Min sketch over SrcAddr, weight Bytes*SamplingRate (viz-ch.json:233) */
    FA_KEYS_DSTADDR_CMS = 4u, /* same over DstAddr (viz-ch.json:479) */
    FA_KEYS_ADDR_PORT_PROTO = 8u, /* exact (Date,Timeslot,SrcAddr,DstPort,Proto) -> sum(Bytes), sum(Packets), count():
                                     second concurrent key set of BASELINE config 5, same Date/Timeslot rule as
                                     flows_5m (create.sh:92-110); rows via fa_*_window_app */
    FA_KEYS_PORT_HIST = 16u,      /* exact sum(Bytes*SamplingRate), count() GROUP BY SrcPort and GROUP BY DstPort
                                     (viz-ch.json:358,604); dense below 65536, hashed above (UInt32 column) */
    FA_KEYS_MINUTE_SERIES = 32u   /* sum(Bytes*SamplingRate) GROUP BY toStartOfMinute(TimeFlowStart) (viz-ch.json:74) */
};

typedef struct {
    int32_t device;               /* HIP device ordinal */
    uint32_t window_secs;         /* 300 = toStartOfFiveMinute (create.sh:96); must divide 86400 */
    uint32_t subwindow_secs;      /* 0, or a divisor of window_secs (60 = toStartOfMinute, viz-ch.json:74):
                                     rows are kept per sub-bucket so sliding windows can be formed */
    uint32_t table_capacity_log2; /* slots of the device group-by table (64 B each); 0 -> 20 */
    uint32_t cms_depth;           /* 0 -> 4 */
    uint32_t cms_width_log2;      /* 0 -> 20 */
    uint64_t cms_seed;
    uint32_t key_sets;            /* 0 -> FA_KEYS_AS_PAIR */
    int32_t framed;               /* 1: each record is varint(len)||payload (-proto.fixedlen=true,
                                     mocker.go:98-101); 0: bare payload (mocker.go:96-97) */
    uint32_t max_batch_records;   /* upper bound on n per ingest call; 0 -> 1<<24; at most (1<<25)-1 (a call whose records
                                     leave as wide tuples is split into launches of <= 1<<24) */
    uint32_t topk_capacity_log2;  /* slots of each distinct-address set behind fa_topk (32 B each); 0 -> 20 */
    uint32_t wide_capacity_log2;  /* slots of the wide-key table (64 B each) behind FA_KEYS_ADDR_PORT_PROTO /
                                     PORT_HIST / MINUTE_SERIES; 0 -> 20; grows by itself like the flows_5m table */
    uint32_t topk_mode;           /* ABI 7.  FA_TOPK_EXACT (0): fa_topk ranks EVERY address ever ingested (the ranking the dashboards
                                     compute, viz-ch.json:233,479) - the distinct-address sets hold every key (2^(universe + 1) slots)
                                     and the ingest path looks each non-repeating address up in them.
                                     FA_TOPK_CANDIDATES (1): the standard Count-Min heavy-hitter contract, made deterministic per
                                     ingest launch ("batch" t = one launch, fa_stats.kernel_launches):
                                       R_t = R_(t-1) u { x in batch t : estimate_(t-1)(x) >= theta_(t-1) },
                                       theta_t = max(lower edge of the estimate bin (64 octaves x 32 steps) that holds rank
                                                 topk_track among R_t's estimates [0 while |R_t| < topk_track],
                                                 total weight_t >> (topk_capacity_log2 - 2), 1);
                                     (Launch boundaries are the library's: one fa_ingest / fa_ingest_device call is ONE launch
                                     unless it exceeds max_batch_records or 2^24 wide-tuple records, or is the first large call
                                     of a ctx with FA_KEYS_ADDR_PORT_PROTO - those are split.  R is therefore a function of the
                                     stream, the caller's batches AND the configuration; what is guaranteed for every split is
                                     the containment below, and bit-for-bit reproducibility for a fixed configuration.)
                                     (A chunk of a sketch fold from columns or from parts - fa_sketch_fold_columns_device,
                                     fa_raw_restore - IS a batch too: a fold of n records is cut into chunks of at most
                                     max_batch_records, in fa_raw_restore also at part boundaries and at the other selected
                                     destinations' caps; each chunk is admitted against the bits of the boundary before it and
                                     ends in a boundary of its own, whether the batch before it was an ingest launch or a chunk.)
                                     fa_topk ranks R - every key whose estimate stood at or above the running topk_track-th
                                     estimate at a batch boundary and that occurred again afterwards: on a stream whose heavy
                                     hitters recur in every batch the same rows as the exact mode (BASELINE config 3: checked),
                                     without the 2 x 2 GiB of sets in the ingest path.  Nothing is admitted during the first
                                     batch of a ctx.  Restated in oracle/pyoracle.py (topk_candidates).  Sizing: the weight term
                                     of theta bounds R by the keys whose ESTIMATE reaches total >> (topk_capacity_log2 - 2) - at
                                     most 2^(topk_capacity_log2 - 2) true ones plus what the sketch's noise (about
                                     total >> cms_width_log2 per counter) lifts over it: keep cms_width_log2 >= topk_capacity_log2
                                     - 1, or a stream of many light keys fills R and fa_topk reports FA_ERR_TABLE_FULL. */
    uint32_t topk_track;          /* candidates mode: the rank the threshold follows (fa_topk serves k <= topk_track); 0 -> 256.
                                     Addresses above the threshold take the slower path through the set: the cost grows with it
                                     (BASELINE config 3: 1.02 / 1.16 / 1.20 ms per launch at 16 / 128 / 1024) */
    uint32_t reserved[1];
} fa_config;
enum { FA_TOPK_EXACT = 0, FA_TOPK_CANDIDATES = 1 };

/* One flows_5m row, scalar columns (create.sh:70-90). */
typedef struct {
    uint32_t date;     /* toDate(TimeReceived), days since 1970-01-01 UTC (create.sh:66) */
    uint32_t timeslot; /* start of the (sub)window, seconds (create.sh:96) */
    uint32_t src_as, dst_as, etype, _pad;
    uint64_t bytes, packets, count; /* sum(Bytes), sum(Packets), count() - wrap mod 2^64 */
} fa_row5m;

/* One row of the (SrcAddr,DstPort,Proto) rollup (FA_KEYS_ADDR_PORT_PROTO). */
typedef struct {
    uint32_t date;        /* toDate(TimeReceived) */
    uint32_t timeslot;    /* start of the (sub)window, seconds */
    uint8_t src_addr[16]; /* FixedString(16) (create.sh:12) */
    uint32_t dst_port, proto;
    uint64_t bytes, packets, count;
} fa_row_app;

/* GROUP BY SrcPort / DstPort (viz-ch.json:358,604). */
typedef struct {
    uint32_t port, _pad;
    uint64_t weight; /* sum(Bytes*SamplingRate), wraps mod 2^64 */
    uint64_t count;  /* rows with this port (a port whose rows all have weight 0 is still a group) */
} fa_port_row;

/* GROUP BY toStartOfMinute(TimeFlowStart) (viz-ch.json:74). */
typedef struct {
    uint32_t minute; /* start of the minute, seconds (TimeFlowStart narrowed to DateTime, create.sh:40) */
    uint32_t _pad;
    uint64_t weight; /* sum(Bytes*SamplingRate) */
    uint64_t count;
} fa_minute_row;

/* One row of the `flows` table (create.sh:7-27): the 15 projected columns. */
typedef struct {
    uint64_t time_received, time_flow_start, sampling_rate, bytes, packets;
    uint32_t sequence_num, src_as, dst_as, etype, proto, src_port, dst_port;
    uint32_t status; /* 0 = ok, 1 = malformed record (all other members 0) */
    uint8_t sampler_address[16], src_addr[16], dst_addr[16]; /* FixedString(16) */
} fa_flow_row;

/* Device-resident struct-of-arrays projection (the flows_raw analogue in HBM).
 * Every member is a DEVICE pointer to an array of n elements, owned by the ctx
 * and valid until the next fa_decode_device / fa_destroy on that ctx. */
typedef struct {
    const uint64_t *time_received, *time_flow_start, *sampling_rate, *bytes, *packets;
    const uint32_t *sequence_num, *src_as, *dst_as, *etype, *proto, *src_port, *dst_port;
    const uint8_t *sampler_address, *src_addr, *dst_addr; /* 16 B per record */
    const uint8_t* status;                                /* 0 ok, 1 malformed */
} fa_columns;

typedef struct {
    uint64_t records_ok;     /* decoded and aggregated */
    uint64_t records_bad;    /* malformed, dropped (inserter.go:125-126) */
    uint64_t records_slow;   /* handled by the generic (non-LDS) device parser */
    uint64_t bytes_in;       /* wire bytes ingested */
    uint64_t batches;
    uint64_t table_used;     /* occupied group-by slots */
    uint64_t table_capacity;
    uint64_t kernel_ns;        /* device time of the last ingest kernel launch (hipEvent) */
    uint64_t kernel_ns_total;  /* summed over every ingest kernel launch */
    uint64_t kernel_launches;
    uint64_t batch_ns_total;   /* tile kernel .. aggregation kernel, summed over every ingest launch */
    uint64_t records_direct;   /* records that took the direct device-wide-table path */
    uint64_t records_retried;  /* records decoded by the order-free second-chance parser */
    uint64_t wide_used;        /* occupied slots of the wide-key table */
    uint64_t wide_capacity;
    uint64_t wave_tile_launches; /* ingest launches that ran the wave-tile kernel (the rest: workgroup-tile kernel) */
    /* ABI 4 */
    uint64_t compact_tuple_launches; /* ... of those, launches that wrote compact 8-byte tuples (the rest: 16-byte ones) */
    uint64_t records_misfit_compact; /* records of compact-tuple launches whose values only a wide tuple holds */
    uint64_t decode_ns_total;        /* fa_decode_device: device time, summed over its launches (hipEvent) */
    uint64_t decode_launches;
    /* ABI 6 */
    uint64_t records_late;           /* records whose time bucket lies below a flows_5m window that fa_close_window /
                                        fa_drop_window(FA_ROWS_5M, timeslot) had already closed when they arrived.  They are
                                        aggregated like any other record (a later read of that timeslot shows them - what a
                                        late INSERT into flows_5m does, create.sh:70-90); the count tells the consumer that a
                                        closed window has been re-opened. */
    /* the wide log (FA_KEYS_ADDR_PORT_PROTO on a stream that opens a row for most of its records: a launch's 32-byte
     * tuples stay in their scatter segments - a "chunk" - and are folded into the hash table only when more than
     * FA_WIDE_LOG_CHUNKS (default 8) are pending; window reads sort them together with the table's rows).  Memory bound:
     * at most FA_WIDE_LOG_CHUNKS + 1 pairs of segment buffers of 2 x 32 B x (records of the largest launch) + 6 %, i.e.
     * 9 x 1.14 GiB at max_batch_records = 2^24 - held until fa_destroy.  A pair that cannot be allocated is not an
     * error: the oldest pending chunk is folded early and its buffers are taken over (wide_log_nomem_folds). */
    uint64_t wide_log_chunks;        /* chunks pending right now */
    uint64_t wide_log_bytes;         /* device bytes of every segment buffer the log holds (pending + recycled) */
    uint64_t wide_log_records;       /* records of the pending chunks (upper bound of their live tuples) */
    uint64_t wide_log_recorded;      /* chunks recorded so far */
    uint64_t wide_log_folded;        /* ... folded into the table by the region-owned kernel */
    uint64_t wide_log_replayed;      /* ... folded through the atomic replay (the table had grown since they were scattered) */
    uint64_t wide_log_dropped;       /* ... dropped whole by a window close (nothing alive above the watermark) */
    uint64_t wide_log_watermark_moves; /* times a close moved a pending chunk's watermark instead of folding it */
    uint64_t wide_log_nomem_folds;   /* chunks folded early because another pair of segment buffers could not be allocated */
    uint64_t wide_log_mode;          /* 1: the next launch keeps its (SrcAddr,DstPort,Proto) tuples in the log */
    /* ABI 7 - candidates mode (fa_config.topk_mode = FA_TOPK_CANDIDATES), SrcAddr then DstAddr: the admission threshold of the last
     * launch boundary and the candidates held at it (0 in the exact mode) */
    uint64_t topk_theta[2];
    uint64_t topk_candidates[2];
    /* launches of the kernel variant that learns a producer's field order per wave (flows_5m alone; chosen while most records of
     * the last launches needed the order-free parser - a producer that does not marshal in field-number order) */
    uint64_t learnt_order_launches;
    /* ABI 8 - where the HOST time of fa_ingest (host buffers) goes, summed over the calls, in nanoseconds: the whole call, of it the
     * wait for a free staging slot (the transfer and the kernels of the call before the last still hold it: the GPU / PCIe side is
     * behind) and the copy into page-locked staging incl. the offsets' narrowing to 32 bits (the consumer's cores are behind) */
    uint64_t host_ingest_ns;
    uint64_t host_stage_wait_ns;
    uint64_t host_stage_copy_ns;
} fa_stats_t;

typedef struct {
    uint8_t key[16]; /* FixedString(16) address */
    uint64_t weight; /* Count-Min estimate of sum(Bytes*SamplingRate) (>= exact) */
} fa_topk_row;

uint32_t fa_abi_version(void);

int fa_create(const fa_config* cfg, fa_ctx** out);
void fa_destroy(fa_ctx*);
const char* fa_last_error(const fa_ctx*); /* ctx may be NULL: last create error */

/* ---- ingest: decode + project + aggregate (the hot path) ---------------- */
/* Host buffers.  buf[0..len) holds n records back to back; offsets (n+1
 * entries, offsets[n]==len) delimit them - one Kafka message value each
 * (mocker.go:103-106).  offsets may be NULL when cfg.framed: the stream is then
 * split on the host by walking the varint length prefixes. */
int fa_ingest(fa_ctx*, const uint8_t* buf, size_t len, const uint64_t* offsets, size_t n);

/* Device-resident buffers (inputs already in HBM).  d_buf: DEVICE pointer to
 * len bytes, 16-byte aligned, followed by >= 32 readable slack bytes; d_offsets: DEVICE pointer to
 * n+1 uint32 offsets relative to d_buf (so len < 4 GiB per call).  Asynchronous
 * on the ctx stream; fa_sync() or any result call waits.
 * ABI 6: d_offsets may be NULL when cfg.framed - the chain of varint(len)-framed records is then cut into records ON THE
 * DEVICE (per 16 KiB block the first frame start is guessed - the first of the block's 256 leading byte positions from which two
 * consecutive frames are non-empty protobuf messages with ascending field numbers that end where their length prefix says -
 * then proven by a fixed-point pass over all blocks, offsets emitted; n is ignored, the call may become several launches).
 * FA_ERR_FRAMING when the bytes are not such a chain ending at len.  A chain whose guesses do not settle in 12 rounds (records
 * longer than several blocks, producers that do not marshal in field order) is copied back and walked on the host - same
 * result, slower.  Several passes over the bytes: a sixth to a third of the rate of a call WITH offsets (which a Kafka consumer
 * has for free: one message = one record) - the path for framed dumps.  fa_ingest (host buffers, offsets == NULL, 1 MiB <= len
 * <= 1 GiB) uses it too; smaller host buffers are walked on the host. */
int fa_ingest_device(fa_ctx*, const void* d_buf, size_t len, const void* d_offsets, size_t n);

/* ABI 8, optional: allocates NOW what the first fa_ingest calls of a ctx would allocate inside the consumer's loop - both
 * page-locked staging slots and their device twins, the deferral lists - for batches of up to `bytes` wire bytes in `records`
 * records (page-locking 2 x 64 MiB costs tens of milliseconds).  A consumer calls it in Setup with its batch bound. */
int fa_reserve_ingest(fa_ctx*, size_t bytes, size_t records);

int fa_sync(fa_ctx*);

/* ---- decode + project only (flows / flows_raw columns) ------------------- */
int fa_decode(fa_ctx*, const uint8_t* buf, size_t len, const uint64_t* offsets, size_t n,
              fa_flow_row* out_rows /* host, n entries */);
int fa_decode_device(fa_ctx*, const void* d_buf, size_t len, const void* d_offsets, size_t n,
                     fa_columns* out);

/* ---- window close: emit flows_5m rows ------------------------------------ */
/* Lists the distinct timeslots currently held, ascending. */
int fa_open_timeslots(fa_ctx*, uint32_t* out, size_t cap, size_t* n_out);
/* Emits the rows of `timeslot` (0xFFFFFFFF = every row) sorted by
 * (date,timeslot,src_as,dst_as,etype) and removes them from the device table.
 * FA_ERR_CAPACITY (nothing removed) if cap is too small; *n_out = rows needed. */
int fa_close_window(fa_ctx*, uint32_t timeslot, fa_row5m* out, size_t cap, size_t* n_out);
/* Same, without removing (peek). */
int fa_read_window(fa_ctx*, uint32_t timeslot, fa_row5m* out, size_t cap, size_t* n_out);
/* Device-side window close for an exchange across GPUs (RCCL all-gather of rows): the window's rows, sorted like
 * fa_read_window's, stay in HBM.  *d_rows: DEVICE pointer to *n_out fa_row5m, owned by the ctx, valid until its next
 * window / ingest call.  With sub-windows the rows are handed out per sub-bucket (not folded).  Nothing is removed. */
int fa_window_rows_device(fa_ctx*, uint32_t timeslot, const void** d_rows, size_t* n_out);
/* Adds n rows that sit in HBM (another rank's fa_window_rows_device, gathered over RCCL) to this ctx's table. */
int fa_merge_rows_device(fa_ctx*, const void* d_rows, size_t n);

/* ---- ABI 5: device-resident window close (every read above is built from these two steps) ------------------------
 * Row kinds and their emit order (what the matching read call returns):
 *   FA_ROWS_5M        fa_row5m      ORDER BY date, timeslot, src_as, dst_as, etype          (fa_read_window)
 *   FA_ROWS_APP       fa_row_app    ORDER BY date, timeslot, src_addr bytes, dst_port, proto (fa_read_window_app)
 *   FA_ROWS_PORT_SRC / _DST  fa_port_row   ORDER BY weight DESC, port                       (fa_top_ports; viz-ch.json:358,604)
 *   FA_ROWS_MINUTE    fa_minute_row ORDER BY minute                                         (fa_minute_series; viz-ch.json:74)
 *   FA_ROWS_TOPK_SRC / _DST  fa_topk_row   ORDER BY weight DESC, key bytes                  (fa_topk; viz-ch.json:233,479)
 *   FA_ROWS_TALKERS_SRC / _DST  fa_talker_row  ORDER BY weight DESC, key bytes, etype       (fa_top_talkers; ABI 8, addition)
 *   FA_ROWS_QUERY_WEIGHT  fa_query_row  ORDER BY weight DESC, value, key bytes, etype          (fa_raw_query_rows, FA_RAW_O_WEIGHT; ABI 8, addition)
 *   FA_ROWS_QUERY_KEY     fa_query_row  ORDER BY value, key bytes, etype                       (fa_raw_query_rows, FA_RAW_O_KEY; ABI 8, addition)
 * Kinds 7, 10 and 11 are unassigned and stay unknown to every call.  The talker kinds need fa_talkers_enable on the ctx that is
 * called (FA_ERR_UNSUPPORTED otherwise, from fa_rows_device / _merge_device / _partition_device / _fetch alike); they are
 * not windowed - timeslot is ignored - and fa_rows_merge_device refuses rows that are not canonical (fa_merge_talkers' rule:
 * FA_ERR_ARG, nothing merged, the outputs untouched).  An exact top k over partitions needs every partition's WHOLE table
 * (fa_rows_device with k = 0), hash-partitioned: fa_group_top_talkers / dist.top_talkers_merged.
 * The query kinds carry the rows of fa_raw_query_rows[_device] through fa_rows_merge_device / _partition_device / _fetch ON ANY
 * CTX, nothing enabled.  The identity of a row is (value, key bytes, etype); weight and count are summed mod 2^64, value is kept;
 * the partition hashes that identity.  A row carries no GROUP BY: ROWS OF DIFFERENT FA_RAW_G_* KINDS ARE NEVER MIXED IN ONE CALL -
 * the caller's duty (SrcPort 80 and DstPort 80 would be summed).  fa_rows_merge_device refuses a row no query produces - etype
 * outside {0, 0x800}; etype 0x800 with a non-zero byte 4..15; value != 0 together with a non-zero key or etype - with FA_ERR_ARG,
 * nothing merged, the outputs untouched.  fa_rows_device answers FA_ERR_UNSUPPORTED for them: it has no place for the group bit;
 * the rows come from fa_raw_query_rows_device(group, order, 0).  The topic-wide read: fa_group_raw_query_rows / dist.raw_query_merged.
 * Multi-GPU window close (one ctx per GPU / Kafka partition, inserter.go:176): every rank calls fa_rows_device,
 * the ranks all-gather the device buffers over RCCL (counts first, no padding), every rank calls
 * fa_rows_merge_device on the concatenation - sum is a commutative monoid, so the result equals the single-ctx
 * result bit for bit (SummingMergeTree collapse, create.sh:70-90) - and fa_drop_window removes what was closed. */
enum {
    FA_ROWS_5M = 0, FA_ROWS_APP = 1, FA_ROWS_PORT_SRC = 2, FA_ROWS_PORT_DST = 3, FA_ROWS_MINUTE = 4,
    FA_ROWS_TOPK_SRC = 5, FA_ROWS_TOPK_DST = 6,
    /* 7: unassigned */
    FA_ROWS_TALKERS_SRC = 8, FA_ROWS_TALKERS_DST = 9,
    /* 10, 11: unassigned (callers and tests rely on fa_row_bytes(10) == 0) */
    FA_ROWS_QUERY_WEIGHT = 12, FA_ROWS_QUERY_KEY = 13
};
size_t fa_row_bytes(int kind); /* bytes of one row of the kind; 0 for an unknown kind */
/* This ctx's result for (kind, timeslot) exactly as the matching read call would return it - the sub-buckets of a
 * sliding window folded, rows in emit order, cut after k rows (k = 0: all; timeslot is ignored by the kinds that
 * are not windowed) - left in HBM.  *d_rows: DEVICE pointer to *n_out rows, owned by the ctx, valid until its next
 * call.  Nothing is removed.  For FA_ROWS_TOPK_* after fa_merge_allreduce / fa_merged_view_set(1) the estimates come
 * from the merged sketch: the union of every rank's k rows then contains the global top k (a key of the global top k
 * ranks at least as high among the keys of any rank that saw it). */
int fa_rows_device(fa_ctx*, int kind, uint32_t timeslot, size_t k, const void** d_rows, size_t* n_out);
/* Merges n rows of `kind` sitting in HBM (several ranks' fa_rows_device results back to back, any order): rows with
 * equal keys are summed (top-k rows: kept once), the result is put into emit order and cut after k rows (0: all).
 * *d_out: DEVICE pointer to *n_out rows, owned by the ctx, valid until its next call.  The ctx's own state is not
 * touched.  FA_ROWS_5M rows must lie on this ctx's bucket grid (FA_ERR_ARG otherwise).  The ctx reads d_rows on its own
 * stream: whatever wrote them (a collective, a copy on another stream) must have completed when the call is made. */
int fa_rows_merge_device(fa_ctx*, int kind, const void* d_rows, size_t n, size_t k, const void** d_out, size_t* n_out);
/* ABI 6 - hash-partitioned window close, for row sets too large to gather on every rank ((SrcAddr,DstPort,Proto): a
 * window of BASELINE config 5 is 16.6 M rows x 56 B PER RANK).  The n rows of `kind` at d_rows (DEVICE; a fa_rows_device
 * result) are regrouped by owner: rank r of `world` owns the keys with (hash(key) >> 32) * world >> 32 == r (the same function of
 * the key on every rank, independent of the row's sums).  *d_out: DEVICE pointer to the n rows, group 0 first (order
 * inside a group unspecified), owned by the ctx, valid until its next fa_rows_partition_device; counts[r] (HOST array of
 * `world` entries) = rows of group r.  The ranks then exchange the groups with ONE all-to-all (RCCL: all_to_all_single
 * with these counts), every rank calls fa_rows_merge_device on what it received - 1 / world of the keys, complete - and
 * emits or gathers only that share; fa_drop_window as usual.  world <= 1024. */
int fa_rows_partition_device(fa_ctx*, int kind, const void* d_rows, size_t n, uint32_t world, const void** d_out, size_t* counts);
/* Copies n rows of `kind` from HBM into the caller's host buffer (cap in rows).  This call and every window read: when `out` is
 * page-locked host memory (hipHostMalloc, or hipHostRegister'ed by the caller - both ends of the buffer are looked at), a
 * result of 1 MiB or more is ONE copy-engine transfer into it (the link's 57 GB/s on MI355X, no host thread involved); into
 * pageable memory the rows are relayed through the ctx's two pinned slots by host threads (54 GB/s). */
int fa_rows_fetch(fa_ctx*, int kind, const void* d_rows, size_t n, void* out, size_t cap);
/* Removes what fa_close_window / fa_close_window_app would remove after emitting `timeslot` (kind FA_ROWS_5M or
 * FA_ROWS_APP): the whole window for tumbling windows and close-all, the oldest sub-bucket when windows slide. */
int fa_drop_window(fa_ctx*, int kind, uint32_t timeslot);
/* ABI 6: removes every (sub-)bucket whose start lies in [timeslot_lo, timeslot_hi) - both on the bucket grid - in one pass:
 * a consumer of TUMBLING windows over sub-buckets closes a whole window with it (fa_drop_window removes one sub-bucket
 * per call, what a sliding consumer wants). */
int fa_drop_range(fa_ctx*, int kind, uint32_t timeslot_lo, uint32_t timeslot_hi);

/* ---- bulk-load sink: flows_5m rows as ClickHouse RowBinary ------------------- */
/* Serialises rows for `INSERT INTO flows_5m FORMAT RowBinary` with the column list of
 * create.sh:70-90: Date (UInt16 days), Timeslot (DateTime = UInt32), SrcAS, DstAS (UInt32),
 * ETypeMap.EType Array(UInt32), ETypeMap.Bytes / .Packets / .Count Array(UInt64) - one element each,
 * what flows_5m_view writes (create.sh:100-103) - then Bytes, Packets, Count (UInt64).  70 bytes per
 * row; replaces the reference's per-row db.Exec (inserter/inserter.go:100-106).  Pure host code, no ctx.
 * Returns FA_ERR_CAPACITY (and the size in *bytes_out) when cap is too small; FA_ERR_ARG for a Date
 * that does not fit UInt16. */
#define FA_ROWBINARY_ROW5M_BYTES 70
int fa_rows_to_rowbinary(const fa_row5m* rows, size_t n, uint8_t* out, size_t cap, size_t* bytes_out);

/* ---- second exact key set: (SrcAddr, DstPort, Proto) ----------------------- */
/* Same contract as fa_read_window / fa_close_window / fa_merge_rows; rows sorted by
 * (date, timeslot, src_addr bytes, dst_port, proto).  Need FA_KEYS_ADDR_PORT_PROTO. */
int fa_read_window_app(fa_ctx*, uint32_t timeslot, fa_row_app* out, size_t cap, size_t* n_out);
int fa_close_window_app(fa_ctx*, uint32_t timeslot, fa_row_app* out, size_t cap, size_t* n_out);
int fa_merge_rows_app(fa_ctx*, const fa_row_app* rows, size_t n);
/* ABI 7: ONE window's rows without the (date, timeslot) every one of them carries - 48 instead of 56 bytes per row over PCIe, which
 * is what a window close of this key set costs (BASELINE config 5: 16.6 M rows per window).  timeslot: a window start (not
 * 0xFFFFFFFF); sliding windows are folded as in fa_read_window_app; same order.  *date_out = toDate(timeslot). */
typedef struct {
    uint8_t src_addr[16];
    uint32_t dst_port, proto;
    uint64_t bytes, packets, count;
} fa_row_app48;
int fa_read_window_app48(fa_ctx*, uint32_t timeslot, fa_row_app48* out, size_t cap, size_t* n_out, uint32_t* date_out);
int fa_close_window_app48(fa_ctx*, uint32_t timeslot, fa_row_app48* out, size_t cap, size_t* n_out, uint32_t* date_out);

/* ---- dashboard read side (not windowed: the dashboard picks $timeFilter) ----- */
/* dst = 0: GROUP BY SrcPort, 1: GROUP BY DstPort.  Every port that occurred, ORDER BY weight DESC
 * (ties: port ascending), cut at k.  Needs FA_KEYS_PORT_HIST. */
int fa_top_ports(fa_ctx*, int dst, size_t k, fa_port_row* out, size_t cap, size_t* n_out);
/* Adds port rows produced by another ctx / rank. */
int fa_merge_ports(fa_ctx*, int dst, const fa_port_row* rows, size_t n);
/* The per-minute series, ORDER BY minute.  Needs FA_KEYS_MINUTE_SERIES. */
int fa_minute_series(fa_ctx*, fa_minute_row* out, size_t cap, size_t* n_out);
int fa_merge_minutes(fa_ctx*, const fa_minute_row* rows, size_t n);
/* Clears the port groups and the minute series (start of a new $timeFilter range). */
int fa_dashboard_reset(fa_ctx*);

/* ---- ABI 8, addition: exact top talkers, grouped as the dashboards do ------------ */
/* The two top-talker panels (viz-ch.json:233 SrcAddr, :479 DstAddr)
 *   SELECT if(EType = 0x800, IPv4NumToString(...first four bytes...), IPv6NumToString(Addr)) AS ip,
 *          sum(Bytes*SamplingRate) AS sumbytes ... GROUP BY ip ORDER BY sumbytes DESC
 * answered exactly (fa_topk ranks by Count-Min estimates).  The group key is the rendered string's preimage:
 * EType == 0x800 -> family 0x800, address bytes 0..3 followed by twelve zero bytes (bytes 4..15 are ignored, as
 * fa_format_addr ignores them); any other EType -> family 0, all 16 bytes (records that differ only in a non-0x800
 * EType are one group).  The same bytes under the two families are two groups.  Only well-formed records count.
 * Opt-in per ctx and additive: no key_sets bit, no change to any other call's result.  It is a SECOND pass over every
 * ingested batch - fa_decode_device on sub-ranges of at most FA_TALK_CHUNK records (environment, read by
 * fa_talkers_enable; default 2^20), each chunk's columns folded into two exact hash tables of their own on the ctx stream.
 * Consequences on an enabled ctx:
 *  - every fa_ingest / fa_ingest_device OVERWRITES the ctx's column block: a fa_columns from an earlier fa_decode_device
 *    is dead after it;
 *  - fa_stats' decode_launches / decode_ns_total (and records_slow, which the decode pass counts too) include the second pass;
 *  - if the fold fails after the ingest itself succeeded (FA_ERR_NOMEM / FA_ERR_TABLE_FULL while a table grows), the ingest
 *    call returns that error, text in fa_last_error: the batch IS in every other aggregate, and in no talker table from
 *    the failing chunk on.
 * Every call below except fa_talkers_enable returns FA_ERR_UNSUPPORTED on a ctx that was not enabled. */
typedef struct {
    uint8_t key[16];   /* canonical: bytes 4..15 zero when etype == 0x800 */
    uint32_t etype;    /* 0x800 (IPv4 branch) or 0: fa_format_addr(key, etype) is the string the panel shows */
    uint32_t _pad;
    uint64_t weight;   /* exact sum(Bytes*SamplingRate), wraps mod 2^64 */
    uint64_t count;
} fa_talker_row;       /* 40 bytes */

typedef struct {
    uint64_t used[2], capacity[2];   /* SrcAddr, DstAddr tables: occupied slots / slots */
    uint64_t records_folded;         /* status == 0 records folded so far */
    uint64_t records_absorbed;       /* (record, direction) updates that ended in a workgroup's LDS cache, not in a global atomic */
    uint64_t grows;                  /* table rebuilds */
    uint64_t fold_launches, fold_ns_total; /* the fold kernel alone, hipEvent */
} fa_talkers_stats_t;

/* Allocates both tables (2^capacity_log2 slots of 64 bytes each; 0 -> 16; 8..30, FA_ERR_ARG otherwise) and the counters.
 * From then on every successful fa_ingest / fa_ingest_device of the ctx also folds its records' addresses - with offsets
 * or without, whatever number of launches the library makes of the call.  The tables grow by themselves (doubling, load
 * kept at or below 1/2; FA_ERR_TABLE_FULL beyond 2^30 slots, before the chunk that would need them is folded).  A second
 * call is FA_ERR_ARG. */
int fa_talkers_enable(fa_ctx*, uint32_t capacity_log2);
/* The same fold for callers that already decode: n records of `cols` - any DEVICE pointers; only src_addr, dst_addr (both
 * 16-byte aligned), etype, bytes, sampling_rate and status are read.  Asynchronous on the ctx stream. */
int fa_talkers_fold_columns_device(fa_ctx*, const fa_columns* cols, size_t n);
/* dst = 0: GROUP BY SrcAddr, 1: DstAddr.  Every group (k = 0) or the first k, ORDER BY weight DESC, ties by key bytes
 * ascending (memcmp), then etype ascending.  Ordered on the device: only the rows returned cross PCIe.
 * FA_ERR_CAPACITY: *n_out = rows needed. */
int fa_top_talkers(fa_ctx*, int dst, size_t k, fa_talker_row* out, size_t cap, size_t* n_out);
/* Adds rows produced by another ctx / rank (sums commute: two partitions merged equal one ctx over both, bit for bit).
 * A row that is not canonical (etype not 0 / 0x800, non-zero bytes 4..15 under 0x800) -> FA_ERR_ARG, nothing is merged. */
int fa_merge_talkers(fa_ctx*, int dst, const fa_talker_row* rows, size_t n);
/* fa_merge_talkers for n rows that already sit in HBM (d_rows: DEVICE pointer - another ctx's fa_rows_device(FA_ROWS_TALKERS_*)
 * result, a share an exchange delivered): checked on the device by the same rule, merged where they are, no staging copy.
 * Synchronous: d_rows is not referenced after the call. */
int fa_merge_talkers_device(fa_ctx*, int dst, const void* d_rows, size_t n);
/* Empties both tables (they keep their size); the counters of fa_talkers_stats go on counting. */
int fa_talkers_reset(fa_ctx*);
int fa_talkers_stats(fa_ctx*, fa_talkers_stats_t* out);

/* ---- ABI 8, addition: exact top talkers for a time range (bucketed tables) ------- */
/* Both top-talker queries read "... FROM flows_raw WHERE $timeFilter GROUP BY ..." with $dateTimeCol = TimeFlowStart
 * (viz-ch.json:66,225,471).  fa_talkers_enable_buckets is fa_talkers_enable with a time axis: the group key becomes
 * (bucket, canonical address, family), bucket = t32 - t32 % bucket_secs with t32 = (uint32_t)TimeFlowStart (the DateTime
 * narrowing of create.sh:40, the rule FA_KEYS_MINUTE_SERIES follows).  bucket_secs >= 1 and divides 86400, FA_ERR_ARG
 * otherwise.  A ctx is enabled at most once, by either call: a second call of either kind is FA_ERR_ARG.  A ctx enabled with
 * plain fa_talkers_enable behaves exactly as before and reads no time column.
 * On a bucketed ctx:
 *  - fa_talkers_fold_columns_device also reads cols->time_flow_start (8-byte aligned; FA_ERR_ARG without it); the capacity
 *    rule is unchanged (a chunk of m records adds at most m keys per table), but a key now occupies one slot PER BUCKET it
 *    was seen in: fa_talkers_stats' used[] counts (bucket, key) slots;
 *  - fa_top_talkers, fa_rows_device(FA_ROWS_TALKERS_*) and fa_group_top_talkers mean "every bucket held": the same result,
 *    byte for byte, as a plain ctx over the same records;
 *  - fa_merge_talkers / fa_merge_talkers_device return FA_ERR_UNSUPPORTED: an fa_talker_row carries no time.  Partitions
 *    meet through rows in HBM (fa_talkers_range_rows_device -> fa_rows_partition_device -> fa_rows_merge_device, which is
 *    what fa_group_top_talkers_range and dist.top_talkers_merged(t_lo, t_hi) do);
 *  - fa_talkers_reset empties everything and keeps bucket_secs.
 * Every call below returns FA_ERR_UNSUPPORTED on a ctx that is not enabled or was enabled without buckets. */
int fa_talkers_enable_buckets(fa_ctx*, uint32_t capacity_log2, uint32_t bucket_secs);
/* The groups of the well-formed records with t_lo <= t32 < t_hi: sums over the buckets mod 2^64, each key once, in
 * fa_top_talkers' order (weight DESC, key bytes, etype), cut after k rows (0: all).  t_lo lies on the bucket grid; t_hi lies
 * on the grid or is 0xFFFFFFFF = no upper bound - the only way to include the last bucket of the axis (so with
 * bucket_secs = 1, where 0xFFFFFFFF is itself on the grid, an EXCLUSIVE bound of 0xFFFFFFFF cannot be expressed: it always
 * means "to the end" - and t_lo = t_hi = 0xFFFFFFFF is the empty range like every t_lo == t_hi, so with bucket_secs = 1 the
 * last second of the axis cannot be read on its own, only together with the one before it: t_lo = 0xFFFFFFFE).  Off-grid
 * values and t_lo > t_hi are FA_ERR_ARG; t_lo == t_hi gives zero rows.  FA_ERR_CAPACITY: *n_out = rows needed.
 * $timeFilter's exact expansion belongs to the Grafana ClickHouse plugin, which is not part of the reference tree.  It is
 * believed to be inclusive at both ends (TimeFlowStart >= from AND TimeFlowStart <= to), so a caller would pass
 * t_hi = to + 1 rounded up to the grid.  This is unverified. */
int fa_top_talkers_range(fa_ctx*, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, fa_talker_row* out, size_t cap, size_t* n_out);
/* The same result left in HBM (*d_rows: DEVICE pointer, owned by the ctx, valid until its next call): the ranged twin of
 * fa_rows_device(FA_ROWS_TALKERS_*).  Its rows go into fa_rows_partition_device / fa_rows_merge_device with kind 8 / 9. */
int fa_talkers_range_rows_device(fa_ctx*, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, const void** d_rows, size_t* n_out);
/* The bucket starts held in either table, ascending (fa_open_timeslots' contract; FA_ERR_CAPACITY: *n_out = needed). */
int fa_talkers_buckets(fa_ctx*, uint32_t* out, size_t cap, size_t* n_out);
/* Removes every bucket that starts below t (on the grid, FA_ERR_ARG otherwise).  Slots are write-once, so both tables are
 * rebuilt into fresh ones of the same size (twice both tables' memory for the duration: both fresh tables are allocated before
 * either is rebuilt, so FA_ERR_NOMEM drops nothing in either direction); used[] is counted again, capacity[] stays.  No floor is remembered: a record that arrives later with a time below t is folded like any other and opens its
 * bucket again - what a late INSERT does to flows_5m.  A consumer that wants it gone drops again. */
int fa_talkers_drop_before(fa_ctx*, uint32_t t);

/* ---- ABI 8, addition: exact top ports for a time range (bucketed port tables) ---- */
/* Both port panels read "... FROM flows_raw WHERE $timeFilter GROUP BY SrcPort" / "DstPort" (viz-ch.json:358,604) with
 * $dateTimeCol = TimeFlowStart.  fa_ports_enable_buckets gives the ctx two hash tables of its own (SrcPort, DstPort; 32-byte
 * slots) whose group key is (bucket, port):
 *  - bucket = t32 - t32 % bucket_secs with t32 = (uint32_t)TimeFlowStart: the DateTime narrowing of create.sh:40, the rule of
 *    FA_KEYS_MINUTE_SERIES and of fa_talkers_enable_buckets;
 *  - port = the whole 32-bit column value (the column is UInt32): 65536 and above are keys like any other, never dropped or
 *    folded together;
 *  - values: sum(Bytes*SamplingRate) mod 2^64 and count(); only status == 0 records count; a group of weight 0 is still a row.
 * bucket_secs >= 1 and divides 86400; capacity_log2 is 0 (-> 16) or 8..30; FA_ERR_ARG otherwise, and for a second enable.
 * The feature takes no key_sets bit, does not depend on FA_KEYS_PORT_HIST, and is independent of the talkers: a ctx may enable
 * either, both or neither.  From the enable on every successful fa_ingest / fa_ingest_device also folds its records' ports in
 * the second pass the talkers use (each chunk is decoded once for every enabled fold; the consequences listed there - the
 * column block is overwritten, decode_launches include the pass, a failing fold fails the call - hold here too).  The tables
 * grow by themselves (doubling, load kept at or below 1/2; FA_ERR_TABLE_FULL beyond 2^30 slots).
 * UNCHANGED: fa_top_ports, fa_merge_ports, fa_dashboard_reset and fa_rows_device(FA_ROWS_PORT_*) keep their meaning.  They read
 * (and clear) the FA_KEYS_PORT_HIST state and nothing else: they never read or clear the bucketed tables, and nothing below
 * reads or clears the FA_KEYS_PORT_HIST state.
 * Every call below except the enable returns FA_ERR_UNSUPPORTED on a ctx that is not enabled. */
typedef struct {
    uint64_t used[2], capacity[2];   /* SrcPort, DstPort tables: occupied (bucket, port) slots / slots */
    uint64_t records_folded;         /* status == 0 records folded so far */
    uint64_t records_absorbed;       /* (record, direction) updates that ended in a workgroup's LDS cache, not in a global atomic */
    uint64_t grows;                  /* table rebuilds that doubled a table */
    uint64_t fold_launches, fold_ns_total; /* the fold kernel alone, hipEvent */
} fa_ports_stats_t;
int fa_ports_enable_buckets(fa_ctx*, uint32_t capacity_log2, uint32_t bucket_secs);
/* The same fold for callers that already decode: n records of `cols` - any DEVICE pointers; only src_port, dst_port, bytes,
 * sampling_rate, status and time_flow_start are read, each naturally aligned (4 / 4 / 8 / 8 / 1 / 8 bytes).  A missing or
 * misaligned column is FA_ERR_ARG.  Asynchronous on the ctx stream. */
int fa_ports_fold_columns_device(fa_ctx*, const fa_columns* cols, size_t n);
/* dst = 0: GROUP BY SrcPort, 1: DstPort, over the well-formed records with t_lo <= t32 < t_hi: sums over the buckets mod 2^64,
 * each port once, in fa_top_ports' order (weight DESC, then port ascending), cut after k rows (0: all).  The range rule is
 * fa_top_talkers_range's, word for word: both bounds on the bucket grid, t_hi = 0xFFFFFFFF = no upper bound (the only way to
 * include the last bucket of the axis), t_lo == t_hi the empty range, off-grid bounds and t_lo > t_hi FA_ERR_ARG.
 * FA_ERR_CAPACITY: *n_out = rows needed. */
int fa_top_ports_range(fa_ctx*, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, fa_port_row* out, size_t cap, size_t* n_out);
/* The same result left in HBM (*d_rows: DEVICE pointer, owned by the ctx, valid until its next call), as rows of kind
 * FA_ROWS_PORT_SRC / _DST for fa_rows_partition_device / fa_rows_merge_device. */
int fa_ports_range_rows_device(fa_ctx*, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, const void** d_rows, size_t* n_out);
/* The bucket starts held in either table, ascending (fa_talkers_buckets' contract; FA_ERR_CAPACITY: *n_out = needed). */
int fa_ports_buckets(fa_ctx*, uint32_t* out, size_t cap, size_t* n_out);
/* Removes every bucket that starts below t (on the grid, FA_ERR_ARG otherwise): fa_talkers_drop_before's contract.  Both tables
 * are rebuilt into fresh ones of the same size, both allocated before either is rebuilt (FA_ERR_NOMEM drops nothing); used[] is
 * counted again, capacity[] stays.  No floor is remembered: a later record with a time below t opens its bucket again. */
int fa_ports_drop_before(fa_ctx*, uint32_t t);
/* Empties both tables (they keep their size and bucket_secs); the counters of fa_ports_stats go on counting. */
int fa_ports_reset(fa_ctx*);
int fa_ports_stats(fa_ctx*, fa_ports_stats_t* out);

/* ---- ABI 8, addition: flows_raw parts built on the device (sorted Native blocks per Date) ---- */
/* flows_raw (create.sh:36-68) is a MergeTree PARTITION BY Date ORDER BY TimeReceived filled by
 * "SELECT toDate(TimeReceived) AS Date, * FROM flows": one inserted block becomes one part per Date, sorted by the narrowed
 * TimeReceived.  A ctx with fa_raw_enable builds exactly that from the decoded columns in HBM.  One PART is one ClickHouse
 * Native block without BlockInfo:
 *   varuint(16) varuint(rows), then per column in the order of create.sh:38-59
 *   varuint(len(name)) name varuint(len(type)) type, rows little-endian values:
 *   Date Date (2 B, t32 / 86400) | TimeReceived, TimeFlowStart DateTime (4 B: the low 32 bits of the UInt64) | SequenceNum UInt32 |
 *   SamplingRate UInt64 | SamplerAddress, SrcAddr, DstAddr FixedString(16) | SrcAS, DstAS, EType, Proto, SrcPort, DstPort UInt32 |
 *   Bytes, Packets UInt64 - 110 payload bytes per row.
 * `INSERT INTO flows_raw FORMAT Native` takes any concatenation of such blocks.  The format is restated from the ClickHouse
 * documentation: no server was available to load it into (the caveat of fa_rows_to_rowbinary).
 * Rows: records with status != 0 are dropped (inserter.go:125-126); inside a part the rows stand in STABLE ascending order of
 * t32 = (uint32_t)TimeReceived (whether MergeTree's own block sort is stable is unverified; stable is deterministic); a part holds
 * one Date; the parts of one chunk come out in ascending Date; a part without rows is never emitted.  Outside the oracle's time
 * domain (TimeReceived >= 2^32) the narrowing above is applied; parity with ClickHouse there is unverified.
 * Opt-in per ctx and additive: no key_sets bit, no change to any other call's result.  On an enabled ctx the second pass of
 * every fa_ingest / fa_ingest_device (the pass of fa_talkers_enable / fa_ports_enable_buckets: each chunk decoded once for
 * every enabled fold, the consequences listed there) also builds the chunk's parts: a chunk is at most chunk_records records
 * (and the other folds' caps), so one ingest call gives parts per (chunk, Date), in build order.  The builder waits for the
 * stream once per chunk (the image's layout depends on the rows per Date).
 * Memory: pending parts accumulate in ONE device image until they are taken - header + 110 bytes per untaken row (at most
 * twice that while the image grows), plus 24 bytes per record of the largest chunk of scratch; kept until fa_raw_reset.
 * A failed allocation is FA_ERR_NOMEM: the chunk's parts are not built, the parts built before stay pending, the ctx stays usable.
 * There is no group or dist door: parts of different partitions are independent parts of one table and need no merge.
 * Every call below except fa_raw_enable returns FA_ERR_ARG (text in fa_last_error) on a ctx that is not enabled. */
typedef struct {
    uint32_t date, t_min, t_max, _pad; /* the part's Date; smallest and largest t32 in it */
    uint64_t rows, offset, bytes;      /* offset / bytes: where the part lies in the bytes returned by the take */
} fa_raw_part;
typedef struct {
    uint64_t records_in, records_bad;  /* records handed to the builder; of them status != 0, dropped */
    uint64_t rows_out, parts_out, bytes_out; /* built so far (rows_out + records_bad == records_in) */
    uint64_t chunks;                   /* non-empty chunks built */
    uint64_t pending_parts, pending_bytes; /* built and not yet taken */
    uint64_t build_ns_total;           /* device time of the order step and of the gather launches, hipEvent (the part list's round
                                          trip to the host and a growth of the image lie between the two and are not counted) */
    uint64_t build_launches;           /* launches those steps queued (5 per chunk + 1 per part) */
} fa_raw_stats_t;
/* Host only, no ctx: bytes of a part of `rows` rows (header + 110 * rows). */
size_t fa_raw_part_bytes(uint64_t rows);
/* Host only, no ctx, the twin of fa_rows_to_rowbinary: n rows of ONE Date with status 0 in ascending t32 -> one part
 * (FA_ERR_ARG otherwise).  FA_ERR_CAPACITY (and the size in *bytes_out) when cap is too small. */
int fa_flow_rows_to_native(const fa_flow_row* rows, size_t n, uint8_t* out, size_t cap, size_t* bytes_out);
/* chunk_records: 0 = default (2^20), at most 2^24.  A second call is FA_ERR_ARG. */
int fa_raw_enable(fa_ctx*, uint32_t chunk_records);
/* The door for columns already in HBM: n records of `cols` - DEVICE pointers, all 15 columns and status, each naturally aligned
 * (8 / 4 / 16 / 1 bytes; FA_ERR_ARG otherwise) - become parts, chunk_records at a time.  n == 0 and chunks without a good
 * record produce no part and return FA_OK.  Synchronous (unlike the talkers' and the ports' doors): the ctx stream has drained when
 * the call returns, so the columns are not referenced after it and may be freed or overwritten at once. */
int fa_raw_build_columns_device(fa_ctx*, const fa_columns* cols, size_t n);
/* Every pending part, in build order, back to back in `out` (one copy; page-locked `out`: one copy-engine transfer), their
 * descriptions in `parts`; the pending parts are cleared.  If either buffer is too small: FA_ERR_CAPACITY, *bytes_out and
 * *n_parts = what is needed, nothing is consumed. */
int fa_raw_take(fa_ctx*, uint8_t* out, size_t cap, size_t* bytes_out, fa_raw_part* parts, size_t parts_cap, size_t* n_parts);
/* The same, the bytes left in HBM (*d_bytes: DEVICE pointer, owned by the ctx, valid until its next ingest / raw call). */
int fa_raw_take_device(fa_ctx*, const void** d_bytes, size_t* bytes_out, fa_raw_part* parts, size_t parts_cap, size_t* n_parts);
/* Drops the pending parts and releases the image and the scratch; the counters of fa_raw_stats go on counting. */
int fa_raw_reset(fa_ctx*);
int fa_raw_stats(fa_ctx*, fa_raw_stats_t* out);

/* ---- ABI 8, addition: LZ4 frames of the flows_raw parts ---------------------------- */
/* fa_raw_take moves 110 bytes per row and is the expensive step of the raw path; the columns are highly redundant (a constant
 * Date, a sorted TimeReceived, address prefixes, a handful of AS / EType / Proto values).  fa_raw_take_lz4 compresses the
 * pending parts in HBM - one wave per 64 KiB block, csrc/lz4.cuh - and copies the compressed bytes.  Each part becomes ONE frame
 * of the LZ4 frame format (restated from the LZ4 frame format specification):
 *   magic 04 22 4D 18 | FLG 0x60 (version 01, independent blocks, no block checksum, no content size, no content checksum, no
 *   dictionary) | BD 0x40 (64 KiB maximum block size) | header checksum 0x82 = (xxHash32(FLG BD) >> 8) & 0xFF, computed |
 *   data blocks: 4-byte little-endian size + data, at most 65536 input bytes each; a block whose LZ4 form would not be smaller
 *   than its input is stored raw with bit 31 of the size set | EndMark 00 00 00 00.
 * Frames stand back to back in build order; a concatenation of frames is a valid LZ4 stream and each frame alone decodes to one
 * whole part.  ClickHouse takes the stream as `Content-Encoding: lz4` on an HTTP insert or as a .lz4 file for INSERT ... FROM
 * INFILE [UNVERIFIED: no server was available, as for the Native part itself].  ClickHouse's own compressed-block framing is not
 * produced.  The bytes are what this encoder finds, not what liblz4 would write; any conforming decoder reads them.
 * Additive: a ctx that never calls these functions runs the code it ran.  Memory, allocated on first use and released by
 * fa_raw_reset / fa_destroy: a 64 KiB slot per block (= the input's size), the frames (to the bound), 40 bytes per block. */
typedef struct {
    uint64_t frames, blocks, stored_blocks; /* compressed so far by this ctx (both doors); blocks stored raw among them */
    uint64_t bytes_in, bytes_out;           /* input bytes; frame bytes (headers, size words and EndMarks included) */
    uint64_t compress_launches;             /* launches queued by compressions (3 each: blocks, scan, pack); a retry adds none */
    uint64_t device_ns;                     /* hipEvent time of the compressions = block_ns + pack_ns */
    uint64_t block_ns, pack_ns;             /* ... of lz4_block_kernel; of the scan and lz4_pack_kernel */
} fa_raw_lz4_stats_t;
/* fa_raw_take with every part delivered as one frame: parts[i].offset / .bytes describe the FRAME inside the bytes returned,
 * rows / date / t_min / t_max are unchanged, the part's raw size is fa_raw_part_bytes(rows).  FA_ERR_CAPACITY: the exact bytes
 * and parts needed come back and nothing is consumed; the compressed bytes are KEPT, so the retry launches no compression unless
 * a part was built in between - such parts are compressed in addition, in order.  fa_raw_take after a failed fa_raw_take_lz4
 * delivers the plain bytes and clears both; after a successful take of either kind nothing is pending.  Synchronous.
 * FA_ERR_ARG (text in fa_last_error) on a ctx without fa_raw_enable. */
int fa_raw_take_lz4(fa_ctx*, uint8_t* out, size_t cap, size_t* bytes_out, fa_raw_part* parts, size_t parts_cap, size_t* n_parts);
/* The same, the frames left in HBM (*d_bytes: DEVICE pointer, owned by the ctx, valid until its next ingest, raw or lz4 call). */
int fa_raw_take_lz4_device(fa_ctx*, const void** d_bytes, size_t* bytes_out, fa_raw_part* parts, size_t parts_cap, size_t* n_parts);
/* n bytes in HBM (d_in: DEVICE pointer) -> one frame in HBM (*d_out: owned by the ctx, valid until its next ingest, raw or lz4
 * call); n == 0 gives header + EndMark, 11 bytes.  Synchronous.  Works on any ctx, fa_raw_enable is not needed: the door for
 * callers that compress something else (RowBinary rows, for instance).  Pending parts and kept frames are not touched. */
int fa_lz4_frame_device(fa_ctx*, const void* d_in, size_t n, const void** d_out, size_t* bytes_out);
/* Host only, no ctx, the twin: a plain greedy encoder into the same frame format (not necessarily the device's bytes).
 * FA_ERR_CAPACITY (and the size in *bytes_out) when cap is too small. */
int fa_lz4_frame(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* bytes_out);
/* Host only: the largest frame n bytes can give (n + 4 per block + 11). */
size_t fa_lz4_frame_bound(size_t n);
/* The counters of this ctx's compressions; works on any ctx (all zero before the first compression). */
int fa_raw_lz4_stats(fa_ctx*, fa_raw_lz4_stats_t* out);

/* ---- ABI 8, addition: loading flows_raw parts ------------------------------------- */
/* The inverse of the two sections above: parts that fa_raw_take / fa_raw_take_lz4 delivered (a file written from them, say) are
 * decoded and read ON THE DEVICE and folded into the ctx's talker and port tables - the state that answers the ranged panels and
 * lives in HBM only - without re-consuming the wire bytes.  `bytes` (HOST memory) is either a concatenation of LZ4 frames of
 * the form above, one part per frame, or a concatenation of plain Native parts; the two are told apart by the first four bytes
 * (a flows_raw block starts with 0x10).  One call: the host walks the frames (one size word per 64 KiB block), ONE copy brings
 * the bytes to HBM, lz4_decode_kernel (csrc/lz4_decode.cuh, one wave per block) decodes every block into a 64 KiB slot,
 * raw_header_check_kernel derives every part's rows from its size and compares its 16 column headers, ONE copy and ONE
 * synchronisation bring every block's and part's verdict back, and only then raw_unpack_kernel turns the parts into column
 * arrays, a chunk at a time, which the folds read through the doors the ingest's second pass uses.
 * Anything else is FA_ERR_FRAMING with the reason and the byte position in fa_last_error: what spill.lz4_frames_decode refuses
 * (no magic, a skippable frame, a wrong version or header checksum, linked blocks, block or content checksums, a content size, a
 * dictionary id, a block above the maximum, a missing EndMark, a truncated block), a block of more than 65536 bytes, a block
 * that breaks the block format (a token, length byte or offset behind its end, literals past its end, offset 0 or past the
 * bytes decoded, more than 65536 decoded bytes, a last sequence with a match length), a block that is not the last of its frame
 * and does not decode to exactly 65536 bytes; a part whose size fits no row count, whose column count, names or types differ, or
 * that is followed by bytes that are no part.  A REFUSED CALL FOLDS NOTHING - every frame, block and header of the call is
 * validated before the first fold is launched - and the ctx stays usable.
 * NOT inspected: the column VALUES (that Date matches TimeReceived, that TimeReceived is sorted).  NOT fed: loading never builds
 * parts again (a ctx with fa_raw_enable gets no pending part from a load) and never touches flows_5m, the wide table or the
 * sketches - fa_raw_load_rollup below ("the rollups from columns and from parts") is the door that feeds flows_5m and the exact
 * dashboard key sets, the minute series among them, from parts; fa_raw_restore ("the sketches from columns and from parts") feeds
 * those, the sketches and the folds in one pass.
 * Memory, allocated on first use, kept until fa_raw_load_reset / fa_raw_reset / fa_destroy: the compressed copy, 64 KiB per block of decoded image,
 * one chunk of columns (117 bytes per row).  FA_ERR_NOMEM leaves the ctx usable; a caller with a large file loads it in
 * pieces cut at frame boundaries. */
typedef struct {
    uint64_t offset, bytes; /* one frame's decoded bytes inside *d_out; offset is a multiple of 65536 */
} fa_lz4_span;
typedef struct {
    uint64_t calls;                   /* fa_lz4_decode_device + fa_raw_columns_device + fa_raw_load (+ fa_raw_load_rollup) calls whose input was accepted */
    uint64_t frames, blocks, stored_blocks;
    uint64_t bytes_in, bytes_decoded; /* input bytes (plain parts included); bytes that left lz4_decode_kernel */
    uint64_t parts, rows_loaded;      /* parts unpacked; rows handed to the folds by fa_raw_load */
    uint64_t launches;                /* kernel launches queued: decode, header check, unpack (the folds count their own) */
    uint64_t decode_ns, unpack_ns, fold_ns; /* hipEvent times of lz4_decode_kernel, raw_unpack_kernel, the fold launches */
} fa_raw_load_stats_t;
/* Host only, no ctx: the C twin of spill.lz4_frames_decode over the step function the kernel runs (lz4_seq_parse).  A
 * concatenation of frames -> their decoded bytes.  FA_ERR_FRAMING for what is listed above; FA_ERR_CAPACITY (and the size
 * needed in *bytes_out) when cap is too small. */
int fa_lz4_decode(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* bytes_out);
/* Frames in HOST memory -> decoded bytes in HBM (*d_out: DEVICE pointer, owned by the ctx, valid until its next load, lz4 or raw
 * call), spans[f] = where frame f's bytes lie.  FA_ERR_CAPACITY (*n_frames = needed) when spans_cap is too small: the host's
 * frame walk finds that before anything is copied, decoded or counted.  n == 0
 * gives zero frames.  Synchronous.  Works on any ctx. */
int fa_lz4_decode_device(fa_ctx*, const uint8_t* in, size_t n, const void** d_out, fa_lz4_span* spans, size_t spans_cap, size_t* n_frames);
/* Every part of the input unpacked into ONE column block (parts in input order, status 0 for every row, the two times
 * zero-extended from 32 bits); no fold.  The block is owned by the ctx and valid until its next decode or load call.  More
 * than 2^24 rows in total is FA_ERR_ARG.  Synchronous.  Works on any ctx. */
int fa_raw_columns_device(fa_ctx*, const uint8_t* bytes, size_t n, fa_columns* out, size_t* rows_out);
/* Every part of the input folded into every enabled fold of the ctx - the talkers, plain or bucketed, and the bucketed ports -
 * in chunks of at most the folds' chunk caps.  FA_ERR_UNSUPPORTED if neither fold is enabled.  Sums commute: a load on top of
 * ingested state adds to it.  Synchronous. */
int fa_raw_load(fa_ctx*, const uint8_t* bytes, size_t n);
/* The counters of this ctx's decodes and loads; works on any ctx (all zero before the first). */
int fa_raw_load_stats(fa_ctx*, fa_raw_load_stats_t* out);
/* Releases the buffers of the doors above (the input's copy, the decoded image, the column chunk) and of the LZ4 compressions; the
 * counters go on counting.  Works on any ctx - fa_raw_reset does the same but needs fa_raw_enable, which a ctx that only loads
 * does not have.  Pointers the doors returned are invalid afterwards. */
int fa_raw_load_reset(fa_ctx*);

/* ---- ABI 8, addition: merging the pending flows_raw parts --------------------------- */
/* What a MergeTree does to its parts after every insert, done to the pending parts before they leave: a ctx emits one part per
 * (chunk, Date), and fa_raw_merge replaces the pending parts by ONE part per Date that has rows, in ascending Date.  Inside a
 * part the rows stand in ascending t32; ties keep the order (build order of the source part, then row order inside it): a
 * stable sort over the parts laid end to end.  If nothing was taken in between, the merged bytes are bit for bit what ONE chunk
 * holding all those records would have built.  The sources are read where they lie (csrc/raw_merge.cuh).
 * Afterwards fa_raw_take, fa_raw_take_device, fa_raw_take_lz4 and fa_raw_take_lz4_device deliver the merged parts; frames kept
 * from a refused fa_raw_take_lz4 are dropped and the next LZ4 take compresses the merged parts; fa_raw_stats shows the merged
 * state in pending_parts / pending_bytes, and rows_out, parts_out, bytes_out and chunks (built so far) do not move.
 * Nothing to do - no pending part, or one part per Date in ascending Date already - is FA_OK without a launch, and `merges`
 * does not move.  A Date with a single source part is moved with a device copy.
 * Memory: the merged image is a second image as large as the pending bytes, allocated before anything changes; the old image is
 * KEPT as the next merge's spare (fa_raw_reset releases it).  Scratch: 16 bytes per pending row (keys and indices in and out),
 * 16 bytes per pending part, the Date list and hipcub's storage.  FA_ERR_NOMEM leaves the pending parts exactly as they were and
 * the ctx usable.  More than 2^31 - 1 pending rows is FA_ERR_ARG (the number in fa_last_error) before anything changes.
 * Synchronous: the ctx stream has drained when the call returns (one synchronisation for the Date list, one at the end).
 * FA_ERR_ARG (text in fa_last_error) on a ctx without fa_raw_enable. */
typedef struct {
    uint64_t merges;               /* calls that changed the pending list */
    uint64_t parts_in, parts_out;  /* pending parts before / after, summed over those calls */
    uint64_t rows, bytes_in, bytes_out;
    uint64_t launches;             /* kernel launches queued by merges (3 for the order + 1 per Date with several sources) */
    uint64_t order_ns, gather_ns;  /* hipEvent time: key extraction + sort + Date list; the gather launches */
} fa_raw_merge_stats_t;
int fa_raw_merge(fa_ctx*);
/* All zero before the first merge; fa_raw_reset releases the merge's buffers, the counters go on counting. */
int fa_raw_merge_stats(fa_ctx*, fa_raw_merge_stats_t* out);

/* ---- ABI 8, addition: the rollups from columns and from parts ---------------------- */
/* In the reference flows_5m is fed by a materialized view that fires on every block inserted into flows_raw
 * (compose/clickhouse/create.sh:92-110): whoever holds flows_raw can get the rollup back (INSERT INTO flows_5m SELECT ... FROM
 * flows_raw), at another granularity too, and the per-minute panel and both port panels read flows_raw itself
 * (viz-ch.json:74,358,604).  These doors are that step: decoded columns - already in HBM, or unpacked from flows_raw parts - are
 * folded into the ctx's flows_5m table and its exact dashboard key sets (FA_KEYS_AS_PAIR, FA_KEYS_ADDR_PORT_PROTO,
 * FA_KEYS_PORT_HIST, FA_KEYS_MINUTE_SERIES) by rollup_fold_kernel (csrc/rollup.cuh), through the table helpers the ingest kernels
 * use: every selected key set's state is what an ingest of the same records leaves, bit for bit, under the ctx's own
 * window_secs / subwindow_secs (parts written by a 300 s ctx re-roll at 3600 s).  Sums commute: a fold on top of ingested state
 * adds to it.  Records with status != 0 are skipped (inserter.go:125-126); a record below a closed flows_5m window is folded
 * and counted in fa_stats.records_late, as an ingested one is.
 * key_sets: 0 = every exact key set the ctx was created with; otherwise a subset of those - a bit the ctx was not created with
 * is FA_ERR_ARG, a sketch bit (FA_KEYS_SRCADDR_CMS, FA_KEYS_DSTADDR_CMS) FA_ERR_UNSUPPORTED: these two doors do not feed the
 * sketches and the distinct-address sets - fa_sketch_fold_columns_device and fa_raw_restore below do.
 * Both doors are synchronous and end in the settle every read starts with: table growth and the replay of parked updates have
 * happened and fa_last_error is meaningful when they return.  fa_stats.records_ok / records_bad / bytes_in do not move (they
 * count wire records); table_used, wide_used, table_capacity, wide_capacity and records_late do, as after any settle.
 * Additive: a ctx that never calls these functions runs the code it ran.  NOT built: a group door (a loaded ctx is a group member
 * like any other), a consumer flag. */
typedef struct {
    uint64_t calls;                   /* fa_rollup_fold_columns_device + fa_raw_load_rollup calls that succeeded */
    uint64_t records_in, records_bad; /* records handed to fold launches; of them status != 0, skipped */
    uint64_t records_folded;          /* records_in - records_bad */
    uint64_t launches;                /* rollup_fold_kernel launches (one per chunk) */
    uint64_t fold_ns;                 /* hipEvent time of those launches */
} fa_rollup_stats_t;
/* n records of `cols` - DEVICE pointers; status and every column the key sets read are needed, and every pointer given must be
 * naturally aligned (8 / 4 / 16 / 1 bytes): FA_ERR_ARG otherwise.  Read: TimeReceived, Bytes, status always; Packets, SrcAS,
 * DstAS, EType (flows_5m); SrcAddr, DstPort, Proto, Packets ((SrcAddr,DstPort,Proto)); SrcPort, DstPort, SamplingRate (ports);
 * TimeFlowStart, SamplingRate (minutes).  n == 0 is FA_OK without a launch.  Chunks of at most max_batch_records and of what the
 * spill buffers hold if every update of a chunk parks.  The columns are not referenced after the call. */
int fa_rollup_fold_columns_device(fa_ctx*, const fa_columns* cols, size_t n, uint32_t key_sets);
/* fa_raw_load's input contract and front half - LZ4 frames or plain Native parts in HOST memory, everything validated before
 * the first fold, FA_ERR_FRAMING with the reason and the byte position, A REFUSED CALL FOLDS NOTHING - and then every chunk of
 * every part through the fold above.  folds != 0: each chunk also goes to the enabled talker and port folds, as fa_raw_load sends
 * it (chunks then also keep to those folds' caps); FA_ERR_UNSUPPORTED if neither fold is enabled.  Counted in fa_raw_load_stats
 * (calls, parts, rows_loaded, unpack_ns; fold_ns there covers every fold of a chunk) and in fa_rollup_stats. */
int fa_raw_load_rollup(fa_ctx*, const uint8_t* bytes, size_t n, uint32_t key_sets, int folds);
/* The counters of this ctx's rollup folds; works on any ctx (all zero before the first call). */
int fa_rollup_stats(fa_ctx*, fa_rollup_stats_t* out);

/* ---- ABI 8, addition: the sketches from columns and from parts ---------------------- */
/* The last piece of a ctx's state that parts could not bring back: the two Count-Min sketches (FA_KEYS_SRCADDR_CMS,
 * FA_KEYS_DSTADDR_CMS) and the distinct-address sets behind fa_topk.  sketch_fold_kernel (csrc/sketch_fold.cuh) takes decoded
 * columns through the helpers every ingest path ends in (cms_add, keyset_offer): weight = Bytes * SamplingRate (u64, wrapping), key =
 * the raw 16 address bytes (the EType plays no part), records with status != 0 skipped.  Sums commute: the sketches are what an
 * ingest of the same records leaves, bit for bit, and a fold on top of ingested state adds to it.  In the exact mode the sets are
 * those of an ingest too; in the candidates mode every chunk is one batch of the contract (fa_config.topk_mode), so a restored
 * ctx equals a ctx that ingested the same records in the same batches.  A fold makes the merged view stale, as an ingest does.
 * fa_stats.records_ok / records_bad / bytes_in / batches / kernel_launches do not move (they count wire records and ingest
 * launches); topk_theta / topk_candidates do.  After fa_raw_restore(key_sets = 0, folds = 1) a ctx equals, read for read, a ctx
 * that ingested the records the parts hold.
 * Additive: a ctx that never calls these functions runs the code it ran.  NOT built: a group door (a restored ctx is a group
 * member like any other), a consumer flag, the fold fused into the parts' unpack. */
typedef struct {
    uint64_t calls;                   /* fa_sketch_fold_columns_device + fa_raw_restore (with a sketch selected) calls that succeeded */
    uint64_t records_in, records_bad; /* records handed to fold launches; of them status != 0, skipped */
    uint64_t records_folded;          /* records_in - records_bad */
    uint64_t batches;                 /* chunks = batches of the candidates contract */
    uint64_t launches;                /* sketch_fold_kernel launches (one per chunk) */
    uint64_t fold_ns;                 /* hipEvent time of those launches */
} fa_sketch_fold_stats_t;
/* n records of `cols` - DEVICE pointers: status, bytes, sampling_rate and the address column of every selected sketch (src_addr,
 * dst_addr) are needed, the others may be null, and every pointer given must be naturally aligned (8 / 4 / 16 / 1 bytes):
 * FA_ERR_ARG otherwise.  key_sets: 0 = every sketch the ctx was created with; otherwise a subset of those - any other bit (an
 * exact key set, a sketch the ctx was created without) is FA_ERR_ARG; a ctx without any sketch: FA_ERR_UNSUPPORTED.  n == 0 is
 * FA_OK without a launch.  Chunks of at most max_batch_records.  Synchronous: it ends in the settle every read starts with; the
 * columns are not referenced after the call. */
int fa_sketch_fold_columns_device(fa_ctx*, const fa_columns* cols, size_t n, uint32_t key_sets);
/* fa_raw_load's input contract and front half - LZ4 frames or plain Native parts in HOST memory, everything validated before
 * the first fold, FA_ERR_FRAMING with the reason and the byte position, A REFUSED CALL FOLDS NOTHING.  key_sets: 0 = everything
 * the ctx was created with, exact key sets and sketches alike; otherwise a subset (FA_ERR_ARG for a bit the ctx lacks).
 * folds != 0: also the enabled talker and port folds, as fa_raw_load feeds them.  Each chunk is unpacked once and goes to the
 * rollup fold (an exact key set selected), the sketch fold (a sketch selected) and the folds; its length is the smallest of the
 * selected destinations' caps, and chunks end at part boundaries.  FA_ERR_UNSUPPORTED when nothing is selected to fold into.
 * Counted in fa_raw_load_stats, fa_rollup_stats and fa_sketch_fold_stats. */
int fa_raw_restore(fa_ctx*, const uint8_t* bytes, size_t n, uint32_t key_sets, int folds);
/* The counters of this ctx's sketch folds; works on any ctx (all zero before the first call). */
int fa_sketch_fold_stats(fa_ctx*, fa_sketch_fold_stats_t* out);

/* ---- ABI 8, addition: ranged loads of flows_raw parts ------------------------------- */
/* flows_raw is PARTITION BY Date ORDER BY TimeReceived (compose/clickhouse/create.sh:36-62): a WHERE on TimeReceived skips the
 * partitions of other Dates and reads only the granules that can hold the range.  The parts carry the same order, and these
 * doors use it: fa_raw_restore_range is fa_raw_restore for the rows with t_lo <= t32 < t_hi, t32 = (uint32_t)TimeReceived, and
 * decodes only the 64 KiB blocks it needs.  A time range is a row range [r_lo, r_hi) of a sorted part, a row range is one
 * contiguous byte slice per column, and the frames' blocks decode alone (FLG 0x60).
 * THE RANGE IS ON THE PRIMARY KEY, TimeReceived, the one ORDER BY serves - not on TimeFlowStart, which the panels filter on
 * (viz-ch.json:66,225).  A caller widens the range by its collectors' delay; the bucketed tables (fa_top_talkers_range,
 * fa_top_ports_range) then answer the exact panel range.  t_hi == 0xFFFFFFFF means "to the end" and includes that second
 * (fa_top_talkers_range's convention); t_lo > t_hi is FA_ERR_ARG; t_lo == t_hi probes and validates but loads nothing (FA_OK).
 * No grid is required.
 * Input: fa_raw_restore's contract - LZ4 frames or plain Native parts in HOST memory, told apart by the first four bytes; ONE
 * copy brings them to HBM.  Three stages, each ending in one synchronisation (csrc/raw_range_plan.h, csrc/raw_range_host.inc):
 *   A probe  block 0 and the last block of every frame are decoded: the decoded size gives the rows, the first bytes are checked
 *            (column count, varuint(rows)) and give Date[0].  A part is SELECTED when rows > 0 and
 *            [Date * 86400, Date * 86400 + 86400) meets the range: partition pruning.
 *   B range  of every selected part the blocks that hold a byte of the 16 column headers or of the TimeReceived column (4 bytes
 *            per row) are decoded; raw_header_check_kernel compares the headers, raw_range_kernel (csrc/raw_range.cuh) makes one
 *            pass over the column: r_lo, r_hi, the first descent, the first row of another Date, t_min and t_max.
 *   C load   of every part with r_lo < r_hi the blocks, not decoded yet, that hold a byte of rows [r_lo, r_hi) of the 14 columns
 *            behind TimeReceived are decoded (the Date values are never needed); then the unpack and fold loop of fa_raw_restore
 *            runs over [r_lo, r_hi).
 * A block is decoded at most once per call.  Plain Native input skips the decodes (stage A reads the host's bytes) and keeps
 * the checks, stage B's kernels and stage C's slice.
 * VALIDATED, before the first fold (A REFUSED CALL FOLDS NOTHING, the ctx stays usable): every frame is walked on the host, as by
 * fa_raw_restore; every block the call decodes (status, and 65536 decoded bytes unless it is its frame's last); every part's
 * row count from its size, column count and varuint(rows); for every selected part all 16 headers, that TimeReceived ascends,
 * and that t32 / 86400 is the part's Date on every row.  A part that is not sorted or holds a row of another Date is
 * FA_ERR_FRAMING, the part and the row in fa_last_error: the range rests on the order, which the whole-file doors never needed
 * (they accept such a part, and go on doing so).  NOT validated: blocks that are not decoded - a corrupt block outside the
 * needed set is not seen -, and of the parts skipped by Date (or without rows) everything beyond their first and last block.
 * Result: afterwards the ctx equals, read for read, a ctx that got fa_raw_restore of parts holding only those rows, in the same
 * order; chunks end at part boundaries, and in the candidates mode each chunk of ranged rows is one batch.  Sums commute: the
 * call adds to ingested state.  key_sets, folds, the mask refusals and FA_ERR_UNSUPPORTED when nothing is selected to fold into:
 * as fa_raw_restore.  Counted in fa_raw_load_stats as a restore is (calls, frames, bytes_in, rows_loaded, launches, unpack_ns,
 * fold_ns; blocks, stored_blocks, bytes_decoded, decode_ns: what went through lz4_decode_kernel; parts: the parts unpacked), in
 * fa_rollup_stats and fa_sketch_fold_stats, and in fa_raw_range_stats.  fa_raw_range_probe counts there too, as the call that loads
 * nothing that it is: calls, frames, bytes_in, blocks, stored_blocks, bytes_decoded, decode_ns and launches move, parts and
 * rows_loaded do not.  A REFUSED call of either door counts nothing - except the launches it had queued and their decode_ns, in both
 * statistics, as a refused call of the whole-file doors does.
 * Memory: that of fa_raw_restore (a slot per block of the input, decoded or not) plus 152 bytes per part.
 * Additive: a ctx that never calls these functions runs the code it ran.  NOT built: copying only the needed compressed bytes
 * (the whole input is copied), a compact image (undecoded slots are allocated), a consumer flag, a range
 * on TimeFlowStart. */
typedef struct {
    uint32_t date, t_min, t_max, _pad; /* Date[0] (0 for a part without rows); t_min / t_max of the rows in range, 0 when none */
    uint64_t rows, r_lo, r_hi;         /* the part's rows; the rows in range are [r_lo, r_hi) (0, 0 for a part that is not selected) */
} fa_raw_range; /* one per part, input order */
typedef struct {
    uint64_t calls;                        /* fa_raw_restore_range + fa_raw_range_probe calls that succeeded */
    uint64_t parts_seen;                   /* parts of those calls = parts_skipped_date + parts_empty + parts with r_lo < r_hi */
    uint64_t parts_skipped_date;           /* rows > 0, but the Date cannot meet the range: only their first and last block were decoded */
    uint64_t parts_empty;                  /* selected by Date but r_lo == r_hi; also a part without rows */
    uint64_t blocks_seen, blocks_decoded;  /* LZ4 blocks of the input; of them sent through lz4_decode_kernel */
    uint64_t rows_seen, rows_loaded;       /* rows of every part; rows handed to the folds (fa_raw_restore_range only) */
    uint64_t launches;                     /* kernel launches queued: decode, probe, header check, range, unpack (the folds count their own) */
    uint64_t probe_ns, range_ns, decode_ns; /* hipEvent times: stage A's kernels; raw_range_kernel; the decode launches of stages B and C */
} fa_raw_range_stats_t;
/* Stages A and B, no fold; works on any ctx.  out[i] describes part i of the input.  FA_ERR_CAPACITY (found by the host's walk,
 * before anything is copied): *n_out = the parts there are.  Synchronous. */
int fa_raw_range_probe(fa_ctx*, const uint8_t* bytes, size_t n, uint32_t t_lo, uint32_t t_hi, fa_raw_range* out, size_t cap, size_t* n_out);
/* Stages A, B and C.  Synchronous: it ends in the settle every read starts with. */
int fa_raw_restore_range(fa_ctx*, const uint8_t* bytes, size_t n, uint32_t t_lo, uint32_t t_hi, uint32_t key_sets, int folds);
/* The counters of this ctx's ranged loads; works on any ctx (all zero before the first call). */
int fa_raw_range_stats(fa_ctx*, fa_raw_range_stats_t* out);

/* ---- ABI 8, addition: selecting rows of flows_raw parts ------------------------------- */
/* "Which flows touched this host, this prefix or this port between 10:05 and 10:20": README.md:144-160's SELECT ... FROM flows_raw
 * with a WHERE.  fa_raw_select reads flows_raw parts as fa_raw_restore_range does - the same input contract (LZ4 frames or plain
 * Native parts in HOST memory), the same three stages, the same validation, the same refusals (an unsorted part or a row of
 * another Date is FA_ERR_FRAMING, the part and the row in fa_last_error), NO DECODE BEYOND stage C's - and delivers, instead of
 * folding them, the ROWS of the time range that meet a filter, as flows_raw parts again.  It works on any ctx: no fa_raw_enable,
 * no fold.
 * The filter.  The time range on TimeReceived, the parts' sort key, ALWAYS applies: t_lo <= (uint32_t)TimeReceived < t_hi;
 * t_hi == 0xFFFFFFFF means "to the end" and includes that second; t_lo == t_hi selects nothing (fa_raw_restore_range's rule).
 * It is what prunes parts and blocks.  Every other condition is named by its bit in `fields`; a member whose bit is clear is
 * not read.  A row matches iff the time range holds, every set condition among FLOW_START, ETYPE and PROTO holds, and
 *     P(Src, Dst) || (EITHER && P(Dst, Src)),
 * P(s, d) = the conjunction of the AS, port and address conditions that are set, the src_* members tested on s, the dst_* members
 * on d.  EITHER is "between A and B in either direction"; with SRC_ADDR alone it is "this host on either side".
 *   FLOW_START   tf_lo <= stored TimeFlowStart (DateTime, 32 bits) < tf_hi, the rule of t_lo / t_hi.  The parts are not sorted by
 *                it: nothing is pruned by it, every row of the TimeReceived range is tested.
 *   SRC_AS, DST_AS, ETYPE, PROTO   equality with the whole UInt32 column value.
 *   SRC_PORT, DST_PORT             lo <= the whole UInt32 column value <= hi (inclusive at both ends).
 *   SRC_ADDR, DST_ADDR             the first prefix_len bits of the stored 16 bytes - from byte 0 on, most significant bit first -
 *                equal those of `addr`; the bits of `addr` behind the prefix are ignored; length 0 matches every row.  The column
 *                holds what the producer stored, whatever the family (README.md:186-191): an IPv4 /24 is prefix_len = 24 over
 *                bytes 0..2, together with ETYPE 0x800 if only that family is wanted.
 *   COUNT_ONLY   nothing is gathered or kept: the parts are still described, with bytes = fa_raw_part_bytes(rows), and *bytes_out
 *                is their sum.
 * FA_ERR_ARG (the reason in fa_last_error): an unknown bit, t_lo > t_hi, tf_lo > tf_hi, a port lo > hi, a prefix length above 128,
 * non-zero _pad.
 * The result: ONE plain Native part per input part that has at least one matching row, in input order, back to back; rows keep the
 * input part's order, so every output part is sorted and holds one Date: each is what INSERT INTO flows_raw FORMAT Native takes and
 * what fa_raw_load, fa_raw_restore and fa_raw_select read.  parts[i]: date, t_min / t_max of the SELECTED rows, rows, offset /
 * bytes inside the selection.  `limit` counts over the call in that order: part by part, and the first rows of the part in which
 * it runs out.  parts_cap below the INPUT's part count is FA_ERR_CAPACITY, found by the host's walk before anything is copied;
 * *n_parts = the parts there are (fa_raw_range_probe's rule).  More than 2^31 - 1 rows in the parts that hold a row of the time
 * range is FA_ERR_ARG before any select launch (the gather's index width, fa_raw_merge's rule).
 * THE SELECTION STAYS IN HBM, owned by the ctx, until the ctx's next fa_raw_select, decode, load, restore or range call
 * (fa_lz4_decode_device, fa_raw_columns_device, fa_raw_load, fa_raw_load_rollup, fa_raw_restore, fa_raw_range_probe,
 * fa_raw_restore_range), fa_raw_load_reset, fa_raw_reset or fa_destroy.  A refused call leaves no selection: the previous one is
 * dropped when the call starts.  FA_ERR_NOMEM leaves the ctx usable.
 * Waits: the three of the ranged load, one for the per-part counts (the output's layout depends on them), one behind the gathers.
 * Counted in fa_raw_load_stats and fa_raw_range_stats as a ranged call that loads nothing: what fa_raw_range_probe moves, plus
 * stage C's decodes and `parts` (the parts with a row of the time range); rows_loaded does not move.  The select's own launches
 * are counted in fa_raw_select_stats alone.
 * Memory, kept until fa_raw_load_reset / fa_raw_reset / fa_destroy: that of the ranged load, 10 bytes per 64 rows of the time
 * range, 8 bytes per selected row, 68 bytes per part with a row of the time range (and as many page-locked), hipcub's storage for
 * one scan, the selection.
 * (A live ctx's pending parts as input: fa_raw_select_pending, below.)  NOT built: a projection of columns, a consumer flag, decoding
 * the predicate's columns first and only the blocks of matching rows afterwards, OR-lists of values, pruning by TimeFlowStart. */
#define FA_RAW_F_FLOW_START 1u
#define FA_RAW_F_SRC_AS 2u
#define FA_RAW_F_DST_AS 4u
#define FA_RAW_F_ETYPE 8u
#define FA_RAW_F_PROTO 16u
#define FA_RAW_F_SRC_PORT 32u
#define FA_RAW_F_DST_PORT 64u
#define FA_RAW_F_SRC_ADDR 128u
#define FA_RAW_F_DST_ADDR 256u
#define FA_RAW_F_EITHER 512u
#define FA_RAW_F_COUNT_ONLY 1024u
#define FA_RAW_F_ALL 2047u
typedef struct {
    uint32_t fields;                 /* FA_RAW_F_* bits; any other bit: FA_ERR_ARG */
    uint32_t t_lo, t_hi;             /* ALWAYS applied: t_lo <= (uint32_t)TimeReceived < t_hi; t_hi = 0xFFFFFFFF: to the end, that
                                        second included; t_lo == t_hi: nothing (fa_raw_restore_range's rule, its text) */
    uint32_t tf_lo, tf_hi;           /* FA_RAW_F_FLOW_START: the same rule on the stored TimeFlowStart (DateTime, 32 bits) */
    uint32_t src_as, dst_as, etype, proto;                          /* equality */
    uint32_t src_port_lo, src_port_hi, dst_port_lo, dst_port_hi;    /* inclusive at both ends; the whole UInt32 column value */
    uint8_t  src_prefix_len, dst_prefix_len, _pad[2];               /* 0 .. 128; _pad must be 0 */
    uint8_t  src_addr[16], dst_addr[16];
    uint64_t limit;                  /* 0: none; else at most this many rows of the call, the FIRST in output order */
} fa_raw_filter; /* 96 bytes */
typedef struct {
    uint64_t calls;                        /* fa_raw_select calls that succeeded */
    uint64_t rows_scanned;                 /* rows of the time ranges: what raw_select_kernel tested */
    uint64_t rows_matched;                 /* of them matching, before `limit` */
    uint64_t rows_out, parts_out, bytes_out; /* delivered (COUNT_ONLY: described) */
    uint64_t launches;                     /* select, scan, totals, emit, gather */
    uint64_t select_ns, emit_ns, gather_ns; /* hipEvent times: raw_select_kernel with the scan; raw_select_emit_kernel; the gathers */
} fa_raw_select_stats_t;
/* Synchronous.  *n_parts = the output parts (FA_ERR_CAPACITY: the input's parts), *bytes_out = the selection's bytes. */
int fa_raw_select(fa_ctx*, const uint8_t* bytes, size_t n, const fa_raw_filter* filter, fa_raw_part* parts, size_t parts_cap, size_t* n_parts, size_t* bytes_out);
/* The ctx's selection where it lies in HBM (nullptr and 0 bytes when there is none). */
int fa_raw_selection_device(fa_ctx*, const void** d_bytes, size_t* bytes_out);
/* Copies the selection out; page-locked `out` takes one copy-engine transfer.  FA_ERR_CAPACITY returns the size in *bytes_out;
 * the selection stays either way. */
int fa_raw_selection_fetch(fa_ctx*, uint8_t* out, size_t cap, size_t* bytes_out);
/* The counters of this ctx's selects; works on any ctx (all zero before the first call). */
int fa_raw_select_stats(fa_ctx*, fa_raw_select_stats_t* out);

/* ---- ABI 8, addition: grouped queries over flows_raw parts ----------------------------- */
/* The ANSWER of a dashboard panel out of stored parts.  The five ClickHouse panels (viz-ch.json:74, 233, 358, 479, 604) are
 *     SELECT <key>, sum(Bytes*SamplingRate) FROM flows_raw WHERE $timeFilter [AND ...] GROUP BY <key> ORDER BY ...
 * with the minute of TimeFlowStart, the rendered SrcAddr, the rendered DstAddr, SrcPort and DstPort as keys.  fa_raw_query reads
 * its input exactly as fa_raw_select does - LZ4 frames or plain Native parts in HOST memory, the same three stages and waits, the
 * same validation and refusals (an unsorted part or a row of another Date is FA_ERR_FRAMING, the part and the row in
 * fa_last_error), no decode beyond stage C's - and folds the rows that meet `where` into one GROUP BY per bit of `groups`, ALL of
 * them in ONE pass over the rows.  It works on any ctx, nothing enabled, and like every range call it drops the ctx's selection.
 * The filter: `where` is fa_raw_filter with its text unchanged (the time range on TimeReceived, the other conditions, EITHER).
 * FA_ERR_ARG (the reason in fa_last_error): what fa_raw_select refuses in a filter; where.limit != 0 or COUNT_ONLY; groups == 0 or
 * a bit outside FA_RAW_G_ALL; an unknown flag; KEEP with `groups` other than those of the result the ctx holds.
 * The values of a group: weight = sum(Bytes*SamplingRate) mod 2^64, count = count().  A group of weight 0 is a row; a kind with no
 * matching row has no rows.
 *   address kinds  key, etype are exactly fa_talker_row's, so fa_format_addr gives the panel's string: EType 0x800 -> etype 0x800,
 *                  bytes 0..3 and twelve zero bytes; any other EType -> etype 0 and all 16 bytes; the same bytes under the two
 *                  families are two groups.  value is 0.
 *   scalar kinds   key is all zeros, etype 0; value = the whole UInt32 column value; MINUTE: the start of the minute in seconds;
 *                  TOTAL: 0.
 * THE RESULT LIES IN HBM, owned by the ctx, until the next fa_raw_query without KEEP (which clears it when it STARTS),
 * fa_raw_query_reset, fa_raw_load_reset, fa_raw_reset or fa_destroy; it survives every other call, fa_raw_select and the restores
 * included.  With KEEP the call's rows are added to the result held (several files, one answer).  Every refusal of the input
 * happens before the first fold launch, so a refused KEEP call leaves the accumulated result as it was; a refused call without
 * KEEP leaves none.
 * Reading: `group` is exactly one bit of the last query's groups (else FA_ERR_ARG; also before any query).  k = 0: every group,
 * else the first k in `order`.  The rows are ordered and cut on the device: only the rows returned cross PCIe.  FA_ERR_CAPACITY
 * puts the rows needed in *n_out.  fa_raw_query_rows_device hands out the same rows in HBM, valid until the ctx's next query call.
 * Rows read with k = 0 are mergeable by sum.
 * The query never reads or writes another aggregate of the ctx: flows_5m, the wide table, the sketches, the talker and port
 * tables and pending raw parts are untouched; it can run on a ctx that is ingesting.
 * Counted in fa_raw_load_stats and fa_raw_range_stats as fa_raw_select is; never in fa_raw_select_stats.
 * Memory, kept until fa_raw_load_reset / fa_raw_reset / fa_destroy: that of the ranged load, 32 bytes per part with a row of the
 * time range (and as many page-locked), two tables of 64-byte slots that start at 2^16 slots and grow until the rows x kinds of
 * a fold launch (at most 2^20 keys) fit at half load - 2^21 slots each for a million rows scanned, whatever matches -, 40 bytes per
 * group of the kind being read, the order's keys.
 * (Pending parts of a live ctx as input: fa_raw_query_pending, below.)  NOT built: decoding only the columns a query names;
 * columns already in HBM as input; sum(Packets),
 * compound keys such as (SrcAS, DstAS), OR-lists; a consumer flag.  (The merge call and the topic-wide doors: "queries over the
 * whole topic", below.) */
#define FA_RAW_G_SRC_ADDR 1u   /* the talker panels' key: fa_talker_row's canonical (key, etype), talkers.cuh's rule */
#define FA_RAW_G_DST_ADDR 2u
#define FA_RAW_G_SRC_PORT 4u   /* the whole UInt32 column value */
#define FA_RAW_G_DST_PORT 8u
#define FA_RAW_G_MINUTE   16u  /* toStartOfMinute(TimeFlowStart): t - t % 60 of the stored 32-bit TimeFlowStart */
#define FA_RAW_G_SRC_AS   32u
#define FA_RAW_G_DST_AS   64u
#define FA_RAW_G_PROTO    128u
#define FA_RAW_G_TOTAL    256u /* one group: every matching row */
#define FA_RAW_G_ALL      511u
#define FA_RAW_Q_KEEP 1u       /* flags: add to the result the ctx holds instead of replacing it */
#define FA_RAW_O_WEIGHT 0      /* weight DESC; ties: value ascending (numeric), key bytes ascending (memcmp), etype ascending */
#define FA_RAW_O_KEY    1      /* value ascending, key bytes ascending, etype ascending */
typedef struct { fa_raw_filter where; uint32_t groups, flags; } fa_raw_query_t;          /* 104 bytes */
typedef struct { uint8_t key[16]; uint32_t etype, value; uint64_t weight, count; } fa_query_row; /* 40 bytes */
typedef struct {
    uint64_t calls;                        /* fa_raw_query calls that succeeded */
    uint64_t rows_scanned;                 /* rows of the time ranges: what raw_query_fold_kernel tested */
    uint64_t rows_matched;                 /* of them matching */
    uint64_t updates;                      /* rows_matched x kinds, summed over the calls */
    uint64_t absorbed;                     /* of them ended in a workgroup's LDS cache */
    uint64_t groups;                       /* occupied slots now: the groups of all kinds of the result held */
    uint64_t grows;                        /* doublings of a table */
    uint64_t launches;                     /* fold, rehash, collect, order and emit launches */
    uint64_t fold_ns, order_ns;            /* hipEvent times: the fold launches; collect, order and emit of the reads */
} fa_raw_query_stats_t;
/* Synchronous. */
int fa_raw_query(fa_ctx*, const uint8_t* bytes, size_t n, const fa_raw_query_t* q);
int fa_raw_query_rows(fa_ctx*, uint32_t group, int order, size_t k, fa_query_row* out, size_t cap, size_t* n_out);
int fa_raw_query_rows_device(fa_ctx*, uint32_t group, int order, size_t k, const void** d_rows, size_t* n_out);
/* Drops the result (the tables keep their size); FA_OK on a ctx that never queried. */
int fa_raw_query_reset(fa_ctx*);
/* The counters of this ctx's queries; works on any ctx (all zero before the first call). */
int fa_raw_query_stats(fa_ctx*, fa_raw_query_stats_t* out);

/* ---- ABI 8, addition: queries over the whole topic -------------------------------------- */
/* One ctx answers for one Kafka partition; a panel asks about the topic.  Three layers, each usable alone:
 *  1. the row kinds FA_ROWS_QUERY_WEIGHT / _KEY (above): query rows through the exchange steps of the window close;
 *  2. fa_raw_query_merge_device / _rows: n rows of ONE kind are ADDED to the result this ctx holds.  Only another ctx's
 *     fa_raw_query_rows[_device](group, any order, k = 0) gives mergeable rows (a cut result lacks groups).  Afterwards
 *     fa_raw_query_rows of this ctx answers for both, and a later fa_raw_query / fa_raw_query_pending with KEEP goes on adding.
 *     `group` is exactly one bit of the held result's groups, else FA_ERR_ARG - also when no result is held: start one with any
 *     query, for instance fa_raw_query_pending over an empty range.  EVERY ROW IS CHECKED BEFORE ANY IS ADDED, a refused call
 *     changes nothing (FA_ERR_ARG): an address kind needs canonical rows (fa_talker_row's rule) with value 0; a scalar kind a zero
 *     key and etype 0; MINUTE value % 60 == 0; TOTAL value 0.  The rows are read where they lie (8-byte aligned; not this ctx's own
 *     result buffers) and not referenced after the call; the host form copies them to HBM first.  raw_query_merge_kernel: one lane
 *     per row, the fold's own key text, the fold's tables and capacity rule (launches of at most 2^20 rows, that many keys reserved
 *     before each).  Counted in fa_raw_query_stats' launches and fold_ns (the add launches are timed as folds) and in
 *     fa_raw_query_merge_stats (fa_raw_query_stats_t has no size argument and cannot grow).
 *  3. the group doors.  fa_group_raw_query_pending runs fa_raw_query_pending(member, q) on every member, KEEP passed through; a
 *     member without fa_raw_enable is FA_ERR_UNSUPPORTED before any member runs.  The members stay the caller's: stored files are
 *     added member by member with fa_raw_query, then this call with KEEP.  fa_group_raw_query_reset: fa_raw_query_reset on every
 *     member.  fa_group_raw_query_rows MERGES WHAT THE MEMBERS HOLD: before anything is collected or exchanged every member must
 *     hold a result whose groups contain `group` (FA_ERR_ARG otherwise, as for a `group` that is not one FA_RAW_G_* bit or a bad
 *     order).  The result equals, BYTE FOR BYTE, fa_raw_query_rows(group, order, k) of ONE ctx whose result covers every member's
 *     rows.  The members' results are not changed and the call is repeatable.  An exact first k cannot be made of the members'
 *     first k (a key that is tenth everywhere can lead overall): every member's whole result of the kind travels in HBM - address
 *     kinds hash-partitioned by owner, merged and cut at k per owner, the n x k rows gathered on one root and merged with the same
 *     cut (fa_group_top_talkers' two stages); scalar kinds, small sets, gathered whole on one root - and k rows cross PCIe.  A
 *     group of one returns its member's first k rows.  FA_ERR_CAPACITY puts the rows needed in *n_out.  A refusal names the
 *     member in fa_group_last_error and in every member's fa_last_error.  FA_VERBOSE prints the steps' times.
 * NOT built: a consumer flag or query protocol in the host program; one exchange for several kinds at once (a read is one kind);
 * sum(Packets), compound keys, OR-lists; a projection of columns. */
typedef struct {
    uint64_t merge_calls;                  /* fa_raw_query_merge_device / _rows calls that added their rows */
    uint64_t rows_merged;                  /* rows they added */
} fa_raw_query_merge_stats_t;
/* Synchronous. */
int fa_raw_query_merge_device(fa_ctx*, uint32_t group, const void* d_rows, size_t n);   /* fa_query_row in HBM */
int fa_raw_query_merge_rows(fa_ctx*, uint32_t group, const fa_query_row* rows, size_t n); /* host rows */
/* Works on any ctx (all zero before the first merge). */
int fa_raw_query_merge_stats(fa_ctx*, fa_raw_query_merge_stats_t* out);

/* ---- ABI 8, addition: the pending flows_raw parts as input ------------------------------ */
/* "Top talkers of the last five minutes": the rows a dashboard asks about most are usually still PENDING in the ingesting ctx - built
 * by fa_raw_enable's second pass, not yet taken - and they lie in HBM in the very layout fa_raw_select's and fa_raw_query's kernels
 * read.  These doors answer from where the rows lie.  All of them need fa_raw_enable (FA_ERR_ARG otherwise).
 * Input: the ctx's pending parts, in build order (what fa_raw_take would deliver now; after fa_raw_merge: one part per Date).
 * NOTHING IS COPIED, DECODED, TAKEN OR CHANGED: after any of these calls the pending parts are byte for byte what they were, and a
 * later fa_raw_take, fa_raw_take_lz4 or fa_raw_merge behaves as if the call had not happened.  Nothing is validated either: the
 * library built every byte itself, sorted.
 * The time range is on TimeReceived with the rule of the ranged loads: t_lo <= t32 < t_hi; t_hi == 0xFFFFFFFF means "to the end"
 * and includes that second; t_lo > t_hi is FA_ERR_ARG; t_lo == t_hi selects nothing.
 * How the range is found (csrc/raw_pending_plan.h, csrc/raw_bounds.cuh): the host holds every pending part's t_min / t_max
 * (fa_raw_part).  From them alone a part is SKIPPED (no row can be in range), WHOLE (every row is) or SEARCHED.  Only for searched
 * parts one kernel runs - raw_bounds_kernel, one wave per part, a 64-ary search of the sorted TimeReceived column: at most
 * ceil(log65(rows)) + 1 loads per lane and bound, against the full pass over the column that untrusted input needs - with one small
 * plan copy, one small copy back and one wait.  A range that covers everything pending, or nothing, launches no such kernel and has
 * no such wait.
 *   fa_raw_pending_probe   fa_raw_range_probe's twin: one fa_raw_range per pending part, build order.  date and rows are always
 *            filled; [r_lo, r_hi) are the rows in range, t_min / t_max those of the rows in range and 0 when there are none; for a
 *            part without a row in range only r_lo == r_hi is promised.  cap below the pending part count: FA_ERR_CAPACITY, *n_out =
 *            the parts there are, nothing launched.
 *   fa_raw_query_pending   fa_raw_query's contract, validation and refusals (the filter's, no limit, no COUNT_ONLY, groups, flags,
 *            the KEEP rule) over the pending rows.  The result lands in the same place and is read by fa_raw_query_rows /
 *            _rows_device, dropped by fa_raw_query_reset, counted in fa_raw_query_stats.  KEEP therefore COMPOSES STORED AND LIVE
 *            DATA: fa_raw_query(bytes of the older files) followed by fa_raw_query_pending(KEEP) is one answer over both.  It reads
 *            and writes no other aggregate, and unlike fa_raw_query it uses no load buffer: THE CTX'S SELECTION STAYS.
 *   fa_raw_select_pending  fa_raw_select's contract: one plain Native part per pending part with a match, rows in input order,
 *            `limit` counted over the call, COUNT_ONLY.  parts_cap below the pending part count is FA_ERR_CAPACITY with *n_parts =
 *            the parts there are, before any launch; more than 2^31 - 1 rows in the parts that hold a row of the time range is
 *            FA_ERR_ARG as in fa_raw_select.  The selection REPLACES the ctx's selection under fa_raw_select's lifetime rule (dropped
 *            when the call starts; a refused call leaves none) and is read by fa_raw_selection_device / _fetch.  It is a copy: it
 *            survives later ingests, merges and takes.
 * No pending parts: FA_OK; a query without KEEP still clears the result held and sets `groups`; a select gives 0 parts.  A pending
 * part of more than 2^32 - 1 rows is FA_ERR_ARG before any launch.
 * Ordering: the pending parts are built on the ctx's stream and these doors launch on it; they are synchronous and end in the waits
 * fa_raw_query / fa_raw_select end in.  A pointer from fa_raw_take_device dies at these calls as at any raw call.
 * Counted in fa_raw_query_stats / fa_raw_select_stats exactly as the file doors count, and in fa_raw_pending_stats; NEVER in
 * fa_raw_load_stats or fa_raw_range_stats: nothing is loaded.
 * Memory, kept until fa_raw_reset / fa_destroy: 48 bytes per searched part (and as many page-locked), plus what the select or the
 * query keeps.
 * Additive: a ctx that never calls these functions runs the code it ran.  NOT built: columns already in HBM (fa_columns) as input,
 * a consumer flag, a projection of columns.  (The topic-wide query: fa_group_raw_query_pending, below.) */
typedef struct {
    uint64_t calls;                        /* probe, query and select calls whose input stood (pending_run succeeded) */
    uint64_t parts_seen;                   /* pending parts of those calls = parts_skipped + parts_whole + parts_searched */
    uint64_t parts_skipped;                /* the host's t_min / t_max say no row can be in range */
    uint64_t parts_whole;                  /* ... that every row is in range */
    uint64_t parts_searched;               /* neither: raw_bounds_kernel found the two positions */
    uint64_t rows_seen, rows_in_range;     /* rows of every pending part; of them in the time range */
    uint64_t bounds_launches, bounds_ns;   /* raw_bounds_kernel launches (at most one per call) and their hipEvent time */
} fa_raw_pending_stats_t;
/* Synchronous. */
int fa_raw_pending_probe(fa_ctx*, uint32_t t_lo, uint32_t t_hi, fa_raw_range* out, size_t cap, size_t* n_out);
int fa_raw_query_pending(fa_ctx*, const fa_raw_query_t* query);
int fa_raw_select_pending(fa_ctx*, const fa_raw_filter* filter, fa_raw_part* parts, size_t parts_cap, size_t* n_parts, size_t* bytes_out);
/* The counters of this ctx's calls over its pending parts (all zero before the first). */
int fa_raw_pending_stats(fa_ctx*, fa_raw_pending_stats_t* out);

/* ---- address rendering of the dashboards (host code, no ctx) ------------------ */
/* The string the top-talker panels group by and display (viz-ch.json:233,479; README.md:186-221):
 *   if(EType = 0x800, IPv4NumToString(reinterpretAsUInt32(substring(reverse(Addr), 13, 4))), IPv6NumToString(Addr))
 * EType 0x0800: the first four bytes of the FixedString(16) in network order, dotted ("192.168.1.1"); any
 * other EType: ClickHouse's IPv6NumToString = the BIND inet_ntop6 rules (longest run of >= 2 zero groups
 * becomes "::", lower-case hex without leading zeros, "::a.b.c.d" / "::ffff:a.b.c.d" for the encapsulated
 * IPv4 forms) - README.md:191 renders the FixedString of 192.168.1.1's little-endian UInt32 as "101:a8c0::".
 * out receives a NUL-terminated string (FA_ADDR_STRLEN bytes always suffice); FA_ERR_CAPACITY if cap is
 * too small. */
#define FA_ADDR_STRLEN 46
int fa_format_addr(const uint8_t addr[16], uint32_t etype, char* out, size_t cap);

/* ---- heavy hitters -------------------------------------------------------- */
/* key_set: FA_KEYS_SRCADDR_CMS or FA_KEYS_DSTADDR_CMS.  The k addresses with the largest Count-Min
 * estimate of sum(Bytes*SamplingRate) (viz-ch.json:233,479) among ALL distinct addresses ingested
 * since the last fa_cms_reset; rows sorted by weight descending, ties by key bytes ascending.
 * Deterministic (independent of ingestion order).  FA_ERR_TABLE_FULL if the distinct-address set
 * overflowed (cfg.topk_capacity_log2). */
int fa_topk(fa_ctx*, uint32_t key_set, size_t k, fa_topk_row* out, size_t cap, size_t* n_out);
/* Adds candidate keys found elsewhere (another GPU / Kafka partition) to this ctx's distinct-address
 * set, so that fa_topk after fa_merge_allreduce ranks the union.  keys: n * 16 bytes (host). */
int fa_topk_merge_keys(fa_ctx*, uint32_t key_set, const uint8_t* keys, size_t n);
int fa_cms_query(fa_ctx*, uint32_t key_set, const uint8_t key[16], uint64_t* weight);
/* Copies the raw sketch (depth * 2^width_log2 uint64) to host. */
int fa_cms_read(fa_ctx*, uint32_t key_set, uint64_t* out, size_t cap_words);
int fa_cms_reset(fa_ctx*, uint32_t key_set); /* sketch and distinct-address set */

/* ---- multi-GPU merge at window close (one ctx per GPU / Kafka partition) --- */
/* Exposes the device-resident mergeable state so the host can run collectives
 * on it (RCCL all-reduce for the dense sketches).  DEVICE pointers. */
typedef struct {
    void* cms_src;      /* depth*2^width_log2 uint64, or NULL */
    void* cms_dst;
    size_t cms_words;
    void* port_hist;        /* 2*65536 entries of {weight, count} uint64 (SrcPort, then DstPort), or NULL */
    size_t port_hist_words; /* 4*65536 */
    /* ABI 4: the MERGED view of the sketches (window close across GPUs): separate buffers of cms_words uint64 that
     * a collective fills with the sum over all ranks - the ctx's own sketches stay untouched, so the merge can be
     * repeated (idempotent) and ingest can go on.  NULL when the key set is off. */
    void* cms_src_merged;
    void* cms_dst_merged;
} fa_device_state;
int fa_device_state_get(fa_ctx*, fa_device_state* out);
/* Declares the merged view valid (1: the caller's collective has filled cms_*_merged with all-rank sums; fa_topk /
 * fa_cms_read / fa_cms_query then answer from it) or stale (0).  Any later ingest or fa_cms_reset makes it stale. */
int fa_merged_view_set(fa_ctx*, int valid);
/* Adds partial rows produced by another ctx/rank (e.g. gathered over RCCL)
 * into this ctx's table: sum is a commutative monoid, so the merged table
 * equals the single-shard table bit for bit. */
int fa_merge_rows(fa_ctx*, const fa_row5m* rows, size_t n);
/* In-library RCCL path: comm is an `ncclComm_t` (librccl.so is bound lazily).  ncclAllReduce(sum, uint64) of the
 * ctx's sketches INTO the merged view (out of place, on the ctx stream) and marks it valid: calling it again - or
 * after more ingest - simply recomputes the view, nothing is ever counted twice.  Sparse state (flows_5m rows, wide
 * rows, port / minute rows) travels as rows: fa_close_window + fa_merge_rows etc. */
int fa_merge_allreduce(fa_ctx*, void* rccl_comm);

int fa_stats(fa_ctx*, fa_stats_t* out);

/* ---- ABI 7: window close of a GROUP of contexts inside one process ----------------------------------------------------
 * The reference's consumer is one process with one goroutine per claimed Kafka partition (inserter.go:167-196, :176); the
 * GPU stage keeps one ctx per (partition, GPU) and ingests without any exchange.  What needs every partition is the window
 * close: the sketches, the top-k, the (SrcAddr,DstPort,Proto) rows have no SummingMergeTree behind them that would sum
 * partial results (flows_5m has: create.sh:70-90 - its rows MAY leave per partition; merged they are fewer and final).
 * A group is that close: the members' results are produced, exchanged and merged in HBM - peer copies between the GPUs
 * (hipMemcpyPeerAsync over xGMI; members on one GPU: device copies), or RCCL for the dense sketches - and one result
 * leaves.  Every result equals, bit for bit, what ONE ctx that ingested all partitions returns from the matching call - with one
 * qualification: in FA_TOPK_CANDIDATES mode every member admits candidates by ITS OWN sketch and threshold (the contract is per
 * ctx and per ingest launch), and the group ranks the UNION of the members' candidates by the merged estimate; a single ctx over
 * all partitions would admit by the merged stream's thresholds.  Both hold every key that stood above its partition's running
 * topk_track-th estimate; they are not the same set in general (equal on streams whose heavy hitters are heavy in every partition).
 * The multi-PROCESS twin (one rank per GPU under torchrun) is flow-pipeline_amd/dist.py over the same ABI 5/6 steps.
 * Threading: a group call uses every member ctx (on host threads of its own, one per member); the caller must not run any
 * other call on a member at the same time (ingest goroutines take a read lock, the closing goroutine the write lock).
 * Errors: a member's failure fails the call, nothing is dropped, and fa_last_error of EVERY member - and
 * fa_group_last_error - name the member and its error. */
typedef struct fa_group fa_group;
enum {
    FA_GROUP_PEER = 0, /* exchange by peer copies; sketches: reduce-scatter + all-gather by peer copies and an add kernel */
    FA_GROUP_RCCL = 1  /* sketches by ncclAllReduce over communicators made with ncclCommInitAll (librccl.so is bound
                          lazily; needs every member on its own GPU - FA_ERR_UNSUPPORTED otherwise); rows still by peer copies */
};
/* ctxs: n contexts (1 <= n <= 1024) with the same window / key-set / sketch / top-k configuration (FA_ERR_ARG otherwise), any
 * placement over the GPUs; a ctx is a member of at most one group at a time.  The contexts stay the caller's: destroy the group
 * first, then them.  What a close needs beyond the members' own buffers (merged sketch views, exchange and partition buffers) is
 * reserved here for members that already hold rows, and - for members that ingest afterwards - when a launch's rows come into
 * being, not inside the first close.  n - 1 host threads live as long as the group. */
int fa_group_create(fa_ctx* const* ctxs, size_t n, uint32_t flags, fa_group** out);
void fa_group_destroy(fa_group*);
const char* fa_group_last_error(const fa_group*); /* group may be NULL: last create error */
size_t fa_group_size(const fa_group*);
int fa_group_transport(const fa_group*); /* FA_GROUP_PEER or FA_GROUP_RCCL */
/* The union of the members' open flows_5m timeslots, ascending (fa_open_timeslots). */
int fa_group_open_timeslots(fa_group*, uint32_t* out, size_t cap, size_t* n_out);
/* Rows of `kind` (FA_ROWS_*) for `timeslot`, merged over the members, in the kind's emit order, cut after k rows (0: all)
 * - fa_read_window / fa_read_window_app / fa_top_ports / fa_minute_series / fa_topk of the whole topic.  `out`: host
 * buffer of cap rows of fa_row_bytes(kind).  Small row sets: every member's result is gathered on one member (they take
 * turns) and merged there.  FA_ROWS_TOPK_*: the sketches are all-reduced first (fa_group_allreduce_sketches), every member
 * ranks its distinct addresses by the MERGED estimate and hands over k rows - exact with respect to the merged sketch.
 * FA_ERR_CAPACITY: *n_out = rows needed. */
int fa_group_read_window(fa_group*, int kind, uint32_t timeslot, size_t k, void* out, size_t cap, size_t* n_out);
/* ... and removes from every member what fa_close_window / fa_close_window_app remove (kind FA_ROWS_5M or FA_ROWS_APP). */
int fa_group_close_window(fa_group*, int kind, uint32_t timeslot, void* out, size_t cap, size_t* n_out);
/* Hash-partitioned form for LARGE row sets ((SrcAddr,DstPort,Proto): 16.6 M rows x 56 B per member and window in BASELINE
 * config 5): every member regroups its rows by owner (fa_rows_partition_device with world = group size), member r receives
 * group r of every member - one peer copy per pair, every xGMI link carries 1 / n of a member's rows -, merges its share
 * (1 / n of the keys, complete) and copies it out over ITS PCIe link while the others do the same.  out receives the shares
 * back to back, share 0 first (share_rows[r] rows each - host array of fa_group_size entries, may be NULL); inside a share
 * the rows are in the kind's emit order; a key appears in exactly one share.  The union equals fa_group_read_window's rows. */
int fa_group_read_window_partitioned(fa_group*, int kind, uint32_t timeslot, void* out, size_t cap, size_t* share_rows, size_t* n_out);
int fa_group_close_window_partitioned(fa_group*, int kind, uint32_t timeslot, void* out, size_t cap, size_t* share_rows, size_t* n_out);
/* Every member's merged sketch view = the sum of all members' sketches (out of place, repeatable: fa_merge_allreduce's
 * contract); fa_topk / fa_cms_read / fa_cms_query of ANY member then answer for the whole topic until it ingests again. */
int fa_group_allreduce_sketches(fa_group*);
/* fa_topk over the whole topic (= fa_group_read_window(FA_ROWS_TOPK_SRC / _DST, 0, k, ...)). */
int fa_group_topk(fa_group*, uint32_t key_set, size_t k, fa_topk_row* out, size_t cap, size_t* n_out);
/* fa_top_talkers over the whole topic, exact (= fa_group_read_window(FA_ROWS_TALKERS_SRC / _DST, any timeslot, k, ...)): every
 * member's table leaves as rows regrouped by owner, member r merges group r of every member and keeps its first k rows (a key
 * lives in exactly one share, with its complete sums), the shares' k rows are gathered on one member and merged with the same
 * cut - all in HBM, k rows cross PCIe.  k = 0: every group.  The result is what fa_top_talkers returns for ONE ctx that folded
 * every partition, byte for byte.  A member without fa_talkers_enable -> FA_ERR_UNSUPPORTED before anything is exchanged (the
 * group's and every member's last error name it).  FA_ERR_CAPACITY: *n_out = rows needed. */
int fa_group_top_talkers(fa_group*, int dst, size_t k, fa_talker_row* out, size_t cap, size_t* n_out);
/* ABI 8, addition: fa_group_top_talkers with every member's rows coming from fa_talkers_range_rows_device(k = 0) instead of
 * fa_rows_device; the result equals fa_top_talkers_range of ONE ctx that folded every partition.  A member that is not
 * bucketed -> FA_ERR_UNSUPPORTED, members with different bucket_secs -> FA_ERR_ARG: both before anything is exchanged, the
 * member named in the group's and every member's last error.  On bucketed members fa_group_top_talkers means every bucket. */
int fa_group_top_talkers_range(fa_group*, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, fa_talker_row* out, size_t cap, size_t* n_out);
/* ABI 8, addition: fa_top_ports_range of ONE ctx that folded every partition.  Port rows are a small set: every member's whole
 * ranged result (fa_ports_range_rows_device, k = 0) is gathered on one member and merged there, cut at k.  A member without
 * fa_ports_enable_buckets -> FA_ERR_UNSUPPORTED, members with different bucket_secs -> FA_ERR_ARG: both before anything is
 * exchanged, the member named in the group's and every member's last error. */
int fa_group_top_ports_range(fa_group*, int dst, uint32_t t_lo, uint32_t t_hi, size_t k, fa_port_row* out, size_t cap, size_t* n_out);
/* Grouped queries over the whole topic: the contract is under "queries over the whole topic" above. */
int fa_group_raw_query_pending(fa_group*, const fa_raw_query_t* q);
int fa_group_raw_query_rows(fa_group*, uint32_t group, int order, size_t k, fa_query_row* out, size_t cap, size_t* n_out);
int fa_group_raw_query_reset(fa_group*);
/* fa_stats summed over the members (kernel_ns: the slowest member's last launch). */
int fa_group_stats(fa_group*, fa_stats_t* out);

/* ---- synthetic producer (mocker/mocker.go:57-106 distribution) ------------ */
enum {
    FA_MOCK_MOCKER = 0,   /* mocker.go:57-91 literally: 9 (SrcAS,DstAS) groups */
    FA_MOCK_ASPAIRS = 1,  /* BASELINE config 2: 65 536 AS pairs x 2 ETypes */
    FA_MOCK_ZIPF = 2,     /* BASELINE configs 3-5: Zipf-distributed addresses */
    FA_MOCK_GOFLOW = 3,   /* ASPAIRS keys in the shape GoFlow marshals an sFlow sample: 33 of the 67 fields of
                             pb-ext/flow.pb.go:57-147 (Type, TimeFlowEnd, SamplerAddress, NextHop, NextHopAS, SrcNet,
                             DstNet, InIf, OutIf, Proto, IP/TCP details, MACs, VLANs, fragment id, flow label), ~165 B */
    FA_MOCK_DISTINCT = 4, /* ASPAIRS shape, every record its own (SrcAS,DstAS) group: table-growth / spill tests */
    FA_MOCK_REVERSED = 5  /* ASPAIRS values, fields marshalled in DESCENDING field-number order: valid proto3 that no
                             canonical-order walk accepts - every record takes the order-free second-chance parser */
};
#define FA_MOCK_MAX_RECORD 256 /* upper bound of one generated record (any mode), framed */
typedef struct {
    uint32_t mode;
    uint32_t framed;    /* -proto.fixedlen */
    uint64_t seed;
    uint64_t n_total;
    uint64_t t0;
    uint32_t span_secs;
    uint32_t per_sec;
    uint32_t zipf_log2_universe;
    uint32_t zipf_s_x100;
} fa_mock_params;
/* Generates records [i0,i0+n) straight into HBM.  d_buf: DEVICE buffer of cap
 * bytes (needs 32 B slack beyond the bytes written); d_offsets: DEVICE n+1
 * uint32.  *bytes_out = bytes written.  Synchronous. */
int fa_mock_generate_device(fa_ctx*, const fa_mock_params*, uint64_t i0, uint64_t n, void* d_buf,
                            size_t cap, void* d_offsets, uint64_t* bytes_out);
/* Host-side twin (same bytes), for feeding fa_ingest. */
int fa_mock_generate_host(const fa_mock_params*, uint64_t i0, uint64_t n, uint8_t* buf, size_t cap,
                          uint64_t* offsets, uint64_t* bytes_out);

#ifdef __cplusplus
}
#endif
#endif
