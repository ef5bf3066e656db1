/*
 * kaiju_gpu.h — C-ABI of the MI355X-native Kaiju classification path.
 *
 * This is the drop-in boundary for the body of the reference's
 * ConsumerThread::doWork() between queue->pop() and the output line
 * (/root/reference/src/ConsumerThread.cpp:632-743): six-frame translation,
 * SEG, MEM / Greedy backward search on the protein FM-index, locate and
 * taxon-id collection run in HIP kernels on gfx950; the caller keeps ingest,
 * the work queue, LCA and output formatting (helpers for the latter two are
 * exported here too so that a host needs nothing else).
 *
 * Plain C: opaque handles, plain pointers and sizes, no C++/torch types, no
 * exit() inside the library.  Every function returns 0 on success or a
 * negative kaiju_gpu_status; kaiju_gpu_strerror() maps it to text.
 *
 * Reference interfaces replaced / mirrored (file:line in /root/reference/src):
 *   kaiju_gpu_index_load        readFMI util.cpp:265-276 -> readIndexes bwt/bwt.c:78-88
 *   kaiju_gpu_index_from_host   the in-memory BWT/FMI/suffixArray structs, bwt/bwt.h:10-22,
 *                               bwt/fmi.h:9-18, bwt/suffixArray.h:10-33
 *   kaiju_gpu_params            Config fields, Config.hpp:33-48 (+ kaiju.cpp:77-80 for -a mem)
 *   kaiju_gpu_create/destroy    ConsumerThread::ConsumerThread ConsumerThread.cpp:6-187
 *   kaiju_gpu_classify_batch    ConsumerThread::doWork ConsumerThread.cpp:630-749, i.e.
 *                               getAllFragmentsBits :190-270, getNextFragment :272-342,
 *                               classify_length :543-628, classify_greedyblosum :424-541,
 *                               ids_from_SI :799-845 (everything up to, not including, lca_from_ids)
 *   kaiju_taxonomy_load         parseNodesDmp util.cpp:79-99
 *   kaiju_taxonomy_lca          lca_from_ids util.cpp:194-263
 *   kaiju_gpu_lca_batch_device  the same on the device (kaiju_gpu_taxonomy_upload: the tree in HBM)
 *   kaiju_finalize_hits         E-value gate ConsumerThread.cpp:500-513, LCA call :538,:625 and the
 *                               C/U decision :724-739
 *   kaiju_gpu_merge_text        the loop of kaiju-mergeOutputs.cpp:110-295, calc_lca :355-399 and
 *                               is_ancestor util.cpp:42-77 on the device
 */
#ifndef KAIJU_GPU_H
#define KAIJU_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The version counts changes that break a caller built against an older header: a struct whose layout changes, a function
   whose arguments or meaning change, a function that goes away.  New functions (and the structs only they use) leave it
   as it is. */
#define KAIJU_GPU_ABI_VERSION 1
#define KAIJU_GPU_MAX_IDS 21   /* ids_from_SI stops once the set holds > max_match_ids (20) ids */

typedef enum {
  KAIJU_GPU_OK = 0,
  KAIJU_GPU_ERR_ARG = -1,        /* bad argument                                  */
  KAIJU_GPU_ERR_IO = -2,         /* file could not be opened / short read          */
  KAIJU_GPU_ERR_FORMAT = -3,     /* .fmi / nodes.dmp content not understood        */
  KAIJU_GPU_ERR_NO_DEVICE = -4,  /* no usable HIP device (the path has NO CPU fallback) */
  KAIJU_GPU_ERR_HIP = -5,        /* a HIP runtime call failed (see strerror)       */
  KAIJU_GPU_ERR_NOMEM = -6,
  KAIJU_GPU_ERR_UNSUPPORTED = -7,/* parameter outside what the kernels implement   */
  KAIJU_GPU_ERR_INDEX_BUG = -8   /* index hits one of the reference's latent bugs  */
} kaiju_gpu_status;

typedef struct kaiju_gpu_index kaiju_gpu_index;   /* FM-index resident in HBM (shareable by contexts) */
typedef struct kaiju_gpu_ctx kaiju_gpu_ctx;       /* one classification stream on one GPU             */
typedef struct kaiju_taxonomy kaiju_taxonomy;     /* host-side nodes.dmp tree                          */

/* mirrors Config (Config.hpp:33-48) */
typedef struct {
  int32_t mode;                 /* 0 = MEM, 1 = GREEDY                               */
  uint32_t min_fragment_length; /* -m, default 11                                    */
  uint32_t mismatches;          /* -e, default 3 (Greedy)                            */
  uint32_t min_score;           /* -s, default 65 (Greedy)                           */
  uint32_t seed_length;         /* -l, default 7 (Greedy)                            */
  int32_t seg;                  /* -x / -X, default on                               */
  int32_t use_evalue;           /* Greedy default on; "-a mem" turns it off          */
  int32_t input_is_protein;     /* -p (Config.hpp:42) and kaijup: reads are protein sequences; unpaired only */
  double min_evalue;            /* -E, default 0.01                                  */
  uint32_t max_matches_SI;      /* 20                                                */
  uint32_t max_match_ids;       /* 20                                                */
} kaiju_gpu_params;

/* what the device produces per read (everything before lca_from_ids) */
typedef struct {
  uint32_t best;                /* MEM: longest match length; GREEDY: best score; 0 = no match */
  uint32_t n_ids;               /* distinct taxon ids collected, <= KAIJU_GPU_MAX_IDS          */
  uint32_t flags;               /* KAIJU_HIT_* bits                                            */
  uint32_t reserved;
  uint64_t taxid[KAIJU_GPU_MAX_IDS]; /* in the reference's traversal (first seen) order       */
} kaiju_gpu_hit;

#define KAIJU_HIT_ID_CAP 1u     /* the 21-id cap ended the traversal (order sensitive case)   */
#define KAIJU_HIT_SI_CAP 2u     /* Greedy: > max_matches_SI equal-score matches existed       */
#define KAIJU_HIT_INEXACT 0x80000000u /* a device-side capacity bound was exceeded for this read (search scratch exhausted
                                   even in the retry pass; the region pool of the exact pass for fragments with more
                                   than 15 SEG regions exhausted): the record is NOT guaranteed to equal the
                                   reference's.  kaiju_gpu_stats.error_flags reports the batch-wide cases: 2 = SEG queue
                                   full, 4 = region pool of the exact pass exhausted, 8 = more than 65536 reads needed
                                   the exact pass                                                              */

/* what the host seam turns a hit into: one output line "C/U \t name \t taxon" */
typedef struct {
  uint64_t taxon;               /* LCA, 0 when unclassified            */
  uint32_t best;                /* column 4 of the -v output           */
  uint8_t classified;           /* 1 = 'C', 0 = 'U'                    */
  uint8_t pad[3];
} kaiju_result;

/* In-memory view of an index as the reference's loader holds it.  All pointers are
   borrowed for the duration of the call only. */
typedef struct {
  int64_t bwtlen;               /* FMI::bwtlen                                              */
  int32_t nseq;                 /* BWT::nseq                                                */
  int32_t alen;                 /* BWT::alen (21 for Kaiju's protein indexes)               */
  const char *alphabet;         /* BWT::alphabet, alen chars, [0] = terminator              */
  const uint8_t *bwt;           /* FMI::bwt, byte-coded (letter, in-block count)            */
  const int32_t *startLcode;    /* FMI::startLcode[alen+1]                                  */
  const uint8_t *sa;            /* suffixArray::sa, ncheck * nbytes big-endian entries      */
  int64_t ncheck;               /* suffixArray::ncheck                                      */
  int32_t chpt_exp, nbytes, pbits; /* suffixArray::chpt_exp / nbytes / pbits                */
  const char *const *ids;       /* suffixArray::ids[nseq], "accession_taxid"                */
} kaiju_gpu_host_index;

typedef struct {
  int64_t bwtlen;
  int32_t nseq, alen, chpt_exp;
  double db_length;             /* Config::db_length = len - nseq (Config.cpp:20)           */
  uint64_t device_bytes;        /* HBM held by the packed index                             */
  uint32_t warnings;            /* KAIJU_IDX_WARN_* bits                                    */
  char alphabet[64];
} kaiju_gpu_index_info;

#define KAIJU_IDX_WARN_SA_SHORT 1u   /* header ncheck one short (suffixArray.c:160 vs bwt.c:115) */
#define KAIJU_IDX_WARN_RANK_BUG 2u   /* bwtlen hits the fmi_chpt_value_with_dir corner case      */

/* work / timing of the last batch of a context */
typedef struct {
  uint64_t n_reads;
  uint64_t n_seg_fragments;      /* fragments that went through the SEG pass              */
  uint64_t n_overflow_retries;   /* reads redone in the retry pass (scratch overflow)     */
  uint64_t error_flags;          /* 0 unless a device-side capacity bound was violated    */
  /* HIP-event times on the stream of the last batch */
  double ms_translate, ms_seg, ms_search, ms_retry, ms_total;
} kaiju_gpu_stats;

int kaiju_gpu_abi_version(void);
const char *kaiju_gpu_strerror(int status);
/* last detailed message of the calling thread (HIP error strings etc.) */
const char *kaiju_gpu_last_error(void);
int kaiju_gpu_device_count(void);

/* ---- index ---------------------------------------------------------- */
int kaiju_gpu_index_load(const char *fmi_path, int device_id, kaiju_gpu_index **out);
int kaiju_gpu_index_from_host(const kaiju_gpu_host_index *view, int device_id, kaiju_gpu_index **out);
/* kaijux / kaijup semantics (ConsumerThreadx.cpp:261-287, README "KaijuX and KaijuP"): a hit collects the
   database SEQUENCES it matches instead of their taxa.  With KAIJU_GPU_IDS_SEQUENCE the ids in kaiju_gpu_hit are
   sequence numbers (kaiju_gpu_index_seq_name() gives the names), first-seen order, capped like taxon ids. */
enum { KAIJU_GPU_IDS_TAXON = 0, KAIJU_GPU_IDS_SEQUENCE = 1 };
int kaiju_gpu_index_load_ex(const char *fmi_or_image_path, int device_id, int id_mode, kaiju_gpu_index **out);
/* The same index on several GPUs of the node (north star: "index replicated per GPU"): parsed and packed once, uploaded to
   devices[0 .. n_devices-1] in turn; out[k] is the replica on devices[k] (free each with kaiju_gpu_index_free). */
int kaiju_gpu_index_load_devices(const char *fmi_or_image_path, const int *devices, int n_devices, int id_mode,
                                 kaiju_gpu_index **out);

/* Device image of an index: the arrays of the HBM layout, packed once on the host and
   written to a file; kaiju_gpu_index_load() recognises such a file by its magic and uploads it without
   parsing or packing anything.  Needs no GPU. */
int kaiju_gpu_index_write_image(const char *fmi_path, const char *image_path);
/* Size in bytes of the .fmi an image was made from (its header remembers it), so that a caller can tell an image of ANOTHER
   index that merely has a newer time stamp (cp -p, rsync -t, restored backups) from a usable one.  Returns 0 or a negative
   status (not an image of this version: KAIJU_GPU_ERR_FORMAT). */
int kaiju_gpu_index_image_source_bytes(const char *image_path, uint64_t *fmi_bytes);

/* Host only: header fields of an image and the number of bytes a load streams from it to the device.  A load of an image
   reads its small arrays (taxon ids, names, count bases) into host memory and moves the arrays that grow with the index - rank
   blocks, sampled suffix-array entries, terminator rows, the k-mer table - from the file to HBM in page-locked pieces
   (KAIJU_GPU_STREAM_PIECE_MB, default 256), two in flight: no host copy of the index exists at any time (the reference maps
   the whole .fmi into every process, readIndexes bwt/bwt.c:78-88).  info->device_bytes = bytes of the packed arrays. */
int kaiju_gpu_index_image_info(const char *image_path, kaiju_gpu_index_info *info, uint64_t *streamed_bytes);

int kaiju_gpu_index_get_info(const kaiju_gpu_index *ix, kaiju_gpu_index_info *info);
/* Diagnostics: a position-sensitive 64-bit digest of every array the index holds in HBM (computed by a kernel, nothing is
   copied back), so that two ways of loading one index - packed on the host, streamed from an image, streamed from the .fmi
   and packed on the device (KAIJU_GPU_FMI_STREAM) - can be compared array by array at any size.  out[]: [0] rank blocks,
   [1] count bases, [2] sampled sequence numbers, [3] taxon ids of the samples, [4] terminator rows, [5] taxon id and [6]
   validity per sequence, [7] k-mer table, [8] k-mer lines, [9] text, [10] full suffix array / 40-bit text positions,
   [11] dense taxon index of every row (row_tax) or - kaiju_gpu_index_layout.row_tax_shift > 0 - of every 2^shift-th row, [12] k (letters of the k-mer table), [13] C[] ; 0 for an array the index
   does not have. */
#define KAIJU_GPU_N_DIGESTS 14
int kaiju_gpu_index_digest(const kaiju_gpu_index *ix, uint64_t *out, uint32_t n_out);
/* Diagnostics: the arrays themselves.  kaiju_gpu_index_get_layout() says how many bytes of each array the index holds in
   HBM (0: it does not have that array) - the digest's twelve in the digest's order, then [12] the taxon id of every dense
   index (tax_of_dense) - and the scalars a reader of those arrays needs; kaiju_gpu_index_read_array() copies bytes
   [offset_bytes, offset_bytes + n_bytes) of array `which` to host memory (a bounds-checked device-to-host copy: no kernel
   runs, nothing is computed).  Digest and reader take pointer and size of an array from one table.  The layouts are those of
   the loader's HBM arrays (kaiju_amd/csrc/kj_core.h: DevIndex); tests compare them element by element with answers derived
   from the index file and its FASTA alone (tests/index_truth.py).  Both calls need a HIP device. */
#define KAIJU_GPU_N_INDEX_ARRAYS 13
enum {
  KAIJU_GPU_ARR_RANK_BLOCKS = 0, KAIJU_GPU_ARR_COUNT_BASES = 1, KAIJU_GPU_ARR_SA_SEQ = 2, KAIJU_GPU_ARR_SA_TAXID = 3,
  KAIJU_GPU_ARR_TERM_ROWS = 4, KAIJU_GPU_ARR_SEQ_TAXID = 5, KAIJU_GPU_ARR_SEQ_VALID = 6, KAIJU_GPU_ARR_KMER_TABLE = 7,
  KAIJU_GPU_ARR_KMER_LINES = 8, KAIJU_GPU_ARR_TEXT = 9, KAIJU_GPU_ARR_SA_FULL = 10 /* wide: the 40-bit text positions */,
  KAIJU_GPU_ARR_ROW_TAX = 11, KAIJU_GPU_ARR_TAX_OF_DENSE = 12
};
typedef struct kaiju_gpu_index_layout {
  uint64_t bytes[KAIJU_GPU_N_INDEX_ARRAYS];
  uint64_t C[22];               /* first row of the suffixes that start with letter c; C[21] = bwtlen                     */
  uint64_t bwtlen, n_sa, sa_skip;
  uint32_t nseq, chpt_exp;
  uint32_t mb_shift;            /* wide: a count base every 2^mb_shift rows                                                */
  uint32_t kmer_k, kline_k;     /* letters of the words of the k-mer table / of the k-mer lines (0: none)                  */
  uint32_t tv_shift;            /* wide: a text position for every 2^tv_shift-th row                                       */
  uint32_t n_dense;             /* entries of tax_of_dense                                                                 */
  uint32_t beyond_lo, beyond_n, beyond_row;   /* KAIJU_IDX_WARN_SA_SHORT: text positions / a row behind the missing sample */
  uint32_t wide;                /* 1 = 64-bit positions (count bases, 16-byte k-mer entries)                               */
  uint32_t row_tax_shift;       /* 0: array 11 is the table of every row, or absent; 1 .. 3: it is the SAMPLED table - entry i = */
                                /* the dense taxon index of row i << row_tax_shift, ((bwtlen >> shift) + 1) * 4 + 64 bytes        */
} kaiju_gpu_index_layout;
int kaiju_gpu_index_get_layout(const kaiju_gpu_index *ix, kaiju_gpu_index_layout *out);
int kaiju_gpu_index_read_array(const kaiju_gpu_index *ix, uint32_t which, uint64_t offset_bytes, uint64_t n_bytes, void *host_out);

/* What the index occupies in HBM, array by array (bytes).  Per index row: rank blocks 2 B; suffix-array sample at exponent e:
   4 / 2^e B of sequence numbers and - indexes below 2^32 rows only - 8 / 2^e B of taxon ids; the k-mer table and its lines
   do not grow with the index (20^k entries).  A refseq-class index (58 G rows, e = 3) is 2.5 B per row = 145 GB + tables. */
typedef struct kaiju_gpu_index_footprint {
  uint64_t rank_blocks;   /* RankBlock64 lines: five bit planes + twenty counts per 64 rows                                */
  uint64_t count_bases;   /* wide layout: the 64-bit counts at the start of every 2^31 rows                               */
  uint64_t sa_seq;        /* sequence number of every sampled suffix-array row                                            */
  uint64_t sa_taxid;      /* taxon id of every sampled row (narrow indexes)                                               */
  uint64_t seq_tables;    /* per database sequence: taxon id, validity, row of its terminator                             */
  uint64_t kmer_table;    /* suffix interval of every k-letter word                                                       */
  uint64_t kmer_lines;    /* the same as 128-byte lines for two end positions each (narrow indexes)                       */
  uint64_t text;          /* the database text (indexes that leave room for it: text verification of long matches)       */
  uint64_t sa_full;       /* ... and position + taxon of every row's suffix, 2 x 4 bytes per row (narrow indexes), or     */
                          /* the 40-bit text position of every 2^s-th row (wide indexes: s = 0 .. 3 by the room left)     */
                          /* + the taxon of every row, 4 bytes each (wide indexes that leave room: KAIJU_GPU_ROW_TAX), or  */
                          /* of every 2^s-th row where only that fits (s = 1 .. 3, KAIJU_GPU_ROW_TAX_SHIFT)               */
  uint64_t other;         /* constant tables                                                                              */
  uint64_t total;
  uint32_t kmer_k, wide;  /* k of the k-mer lines (narrow: a five-letter table stays next to them) or of the table; 1 = 64-bit positions */
} kaiju_gpu_index_footprint;
int kaiju_gpu_index_get_footprint(const kaiju_gpu_index *ix, kaiju_gpu_index_footprint *out);
void kaiju_gpu_index_free(kaiju_gpu_index *ix);

/* ---- classification -------------------------------------------------- */
void kaiju_gpu_default_params(kaiju_gpu_params *p, int mode);
int kaiju_gpu_create(kaiju_gpu_ctx **out, const kaiju_gpu_index *ix, const kaiju_gpu_params *p);
void kaiju_gpu_destroy(kaiju_gpu_ctx *ctx);

/* Host buffers.  seqs: concatenated, already strip()'d ASCII nucleotides (protein letters, either case, when the
   context was created with input_is_protein; such reads have no mate and paired must be 0);
   off[2*n+1]: read r is seqs[off[2r], off[2r+1]) and its mate seqs[off[2r+1], off[2r+2])
   (empty when unpaired).  paired selects the length gate of ConsumerThread.cpp:647-654.
   Blocks until out[0..n) is filled. */
int kaiju_gpu_classify_batch(kaiju_gpu_ctx *ctx, const char *seqs, const uint64_t *off,
                             uint32_t n_reads, int paired, kaiju_gpu_hit *out);

/* Device-resident variant: all pointers are HIP device pointers on the context's
   GPU, work is enqueued on `stream` (a hipStream_t; NULL = the context's own
   stream) and the call returns without synchronising. */
int kaiju_gpu_classify_batch_device(kaiju_gpu_ctx *ctx, const void *d_seqs, uint64_t seq_bytes,
                                    const uint64_t *d_off, uint32_t n_reads, int paired,
                                    kaiju_gpu_hit *d_out, void *stream);
/* Upper bound of the read (mate) lengths of the batches handed to classify_batch_device; it sizes
   per-lane scratch and selects the LDS-staged translation kernel for short reads.  The host-buffer
   entry point measures it itself.  Default 1024. */
int kaiju_gpu_set_max_read_length(kaiju_gpu_ctx *ctx, uint32_t max_read_len);
int kaiju_gpu_synchronize(kaiju_gpu_ctx *ctx);
/* the context's own HIP stream (a hipStream_t): what the device-resident entry points use when they are given NULL; a
   caller that queues its own work behind a batch (a copy, a collective) orders it on this stream */
int kaiju_gpu_get_stream(kaiju_gpu_ctx *ctx, void **stream);
int kaiju_gpu_get_stats(kaiju_gpu_ctx *ctx, kaiju_gpu_stats *stats);
/* Accounting (bench.py's roofline, never a timed launch): with count_ops on, the main search pass of the following
   batches runs the counting instantiation of its lane, which adds up the memory steps of the search as THIS
   implementation performs them; kaiju_gpu_get_op_counts() returns the totals of the last batch:
   [0] k-mer table lookups, [1] UpdateSI steps past the table (bwt.c:160-173), [2] distinct 128-byte rank lines those
   steps (and the Greedy multi-letter steps) touched, [3] LF steps (compactfmi.c:312-336), [4] rank lines of those,
   [5] SA samples read, [6] read descriptors, [7] fragment descriptors, [8] 64-byte peptide windows, [9] terminator
   searches, [10] match records spilled (MEM), [11] hit records written, [12] Greedy multi-letter steps
   (ConsumerThread.cpp:346-395 at one position), [13] queue items read, [14] match records read, [15] queue items
   written, [16] match records written, [17] wave iterations, [18] lane iterations, [19] bytes of the state / queue / task
   records the third-generation Greedy kernels read and write. */
#define KAIJU_GPU_N_OP_COUNTS 20
int kaiju_gpu_set_count_ops(kaiju_gpu_ctx *ctx, int on);
int kaiju_gpu_get_op_counts(kaiju_gpu_ctx *ctx, uint64_t *out, uint32_t n_out);
/* Diagnostics: what the device SEG pass (low-complexity masking, the reference's SeqBufferSeg blast_seg.c:2278-2332) computed,
   fragment by fragment.  ctx: created with input_is_protein and seg; seqs / off: a batch of protein reads in the layout of
   kaiju_gpu_classify_batch (mates empty).  The reads go through the stage 1 of protein reads (fragments between the
   separators, those with a 12-window at the SEG trigger entropy queued) and the queue through the SEG launch of the
   classification path - exact = 0: the SEG pass proper (one wavefront per fragment, or teams of KAIJU_GPU_SEG_TEAM lanes),
   records of 15 regions with 16-bit positions; exact = 1: the SEG kernel of the exact pass with its scratch, region lists of
   any length.  As in kaiju_gpu_classify_batch the longest read of the batch, taken from off[], sizes that scratch (what
   kaiju_gpu_set_max_read_length() says serves the device-resident entry points only).  Nothing is searched; the call blocks.  Per fragment of every read, in the order of the read's fragment list,
   one kaiju_gpu_seg_fragment; regions are (left, right) pairs of int32, positions relative to the fragment's first residue,
   at lr[2 * first .. 2 * (first + n_lr)).  At most frag_cap records and lr_cap pairs are written; *n_frags and *n_lr are
   what the batch has (call again with more room if they exceed the capacities).  kaiju_gpu_get_stats() afterwards reports
   the queued fragments and the error flags of this call. */
#define KAIJU_GPU_SEG_LOST 0xffffffffu   /* n of a fragment whose regions found no room in the pool of the exact pass */
typedef struct {
  uint32_t read;        /* the read the fragment belongs to                                                           */
  uint32_t start, len;  /* its first residue in the read, its length                                                   */
  uint32_t flagged;     /* 1: stage 1 queued it for the SEG pass (0: n, overflow, n_lr are 0)                          */
  uint32_t n;           /* regions: exact = 0 the record's count (<= 15), exact = 1 all of them or KAIJU_GPU_SEG_LOST  */
  uint32_t overflow;    /* exact = 0: the record's flag - more than 15 regions, more raw segments than the scan lists  */
                        /* hold, or more than 65535 residues: the classification path sends such a read to the exact pass */
  uint32_t n_lr;        /* pairs at lr[2 * first ..): exact = 0 all 15 of the record (unused ones 0), exact = 1 n       */
  uint32_t reserved;
  uint64_t first;
} kaiju_gpu_seg_fragment;
int kaiju_gpu_seg_regions(kaiju_gpu_ctx *ctx, const char *seqs, const uint64_t *off, uint32_t n_reads, int exact,
                          kaiju_gpu_seg_fragment *frags, uint64_t frag_cap, uint64_t *n_frags,
                          int32_t *lr, uint64_t lr_cap, uint64_t *n_lr);

/* Diagnostics: the table the SEG kernels take s_Trim's window probabilities from (one double per multiset of letter counts,
   computed on the host once per process) against the device's own arithmetic.  One kernel computes every entry again with
   the function the table replaces and looks it up as the SEG pass does; *entries: entries of the table, *mismatches: those
   whose key, presence or 64-bit pattern differs (0 on a working device).  The environment variable KAIJU_GPU_SEG_TABLE=0,
   read when an index is loaded, makes the SEG kernels of that index compute every window directly; the check still runs. */
int kaiju_gpu_seg_table_check(const kaiju_gpu_index *index, uint64_t *entries, uint64_t *mismatches);

/* Diagnostics: the rule by which the Greedy lane leaves a substitution variant on a few database rows unqueued
   (kj_chain_hopeless), by itself.  A case is what the lane hands the rule: its window of the fragment (win[0] is
   fragment position wq; KAIJU_GPU_CHAIN_WIN bytes - the 64 letters of the window and the slack of the lane's row behind them),
   the variant's match [pz, j] of the fragment, tx = the 16 bytes of database text in front of the match (tx[15] next to it),
   nmm substitutions made so far, sc0 the match's score, thr the score that matters, and the parameters m (min_fragment_length)
   and mismatches.  One kernel, one lane per case, writes out[i] = 1 where the rule says that no item of the chain can hold a
   match of m letters that scores thr, else 0.  No index and no context are needed.  Cases the lane cannot pass (wq < 0, pz < 0,
   j < pz, pz - wq > 63, positions above 65535, mismatches > 8, nmm > mismatches) and more than 2^24 cases give
   KAIJU_GPU_ERR_ARG.  The call blocks; it runs on `device` and leaves the calling thread's current device as it found it. */
#define KAIJU_GPU_CHAIN_WIN 68
typedef struct {
  uint8_t win[KAIJU_GPU_CHAIN_WIN];
  uint8_t tx[16];
  int32_t wq, pz, j;
  int32_t sc0, thr;
  uint32_t nmm, m, mismatches;
} kaiju_gpu_chain_case;
int kaiju_gpu_chain_hopeless_check(int device, const kaiju_gpu_chain_case *cases, uint32_t n_cases, uint8_t *out);

/* Diagnostics: the locate by itself.  Record r is given the suffix-array intervals first[r] .. first[r + 1] - 1 (at most 16:
   rows lo[i] .. lo[i] + len[i] - 1, len[i] >= 1) as the matches a search lane would have left in it, and the call runs the
   locate that a classification of this context would run on this index (the row -> taxon table, the sampled one, or the walk
   to the suffix array's sample) over them: out[r] holds the ids of those rows in the reference's order (ids_from_SI: rows in
   order, the limit max_match_ids tested in front of every row, first seen first) and KAIJU_HIT_ID_CAP where the limit ended
   the traversal.  An interval that leaves the index (or, on an index with 32-bit positions, one whose length does not fit the
   record), a record of more than 16 intervals and a call with more than KAIJU_GPU_LOCATE_MAX_RECORDS records give
   KAIJU_GPU_ERR_ARG.  first[0] must be 0.  The call blocks.  It lets a test meet every alignment of an interval against the
   samples without a read that produces it.  Where a classification would finish its records in the fused post-search pass (MEM
   on an index with 32-bit positions and the row -> taxon table) the call runs k_mem_locate + k_mem_locate_list, the stand-alone
   kernels of the same locate (what KAIJU_GPU_FUSED_POST=0 runs); a context whose search lanes walk to their ids themselves
   (KAIJU_GPU_MEM_LANE=v1 and the like) has no locate kernel: KAIJU_GPU_ERR_UNSUPPORTED. */
#define KAIJU_GPU_LOCATE_MAX_INTERVALS 16
#define KAIJU_GPU_LOCATE_MAX_RECORDS (1u << 24)
int kaiju_gpu_locate_intervals(kaiju_gpu_ctx *ctx, const uint64_t *lo, const uint32_t *len, const uint32_t *first,
                               uint32_t n_records, kaiju_gpu_hit *out);

/* ---- host side of the seam ------------------------------------------- */
int kaiju_taxonomy_load(const char *nodes_dmp_path, kaiju_taxonomy **out);
void kaiju_taxonomy_free(kaiju_taxonomy *t);
/* ids need not be sorted; returns 0 if none of them is in the tree */
uint64_t kaiju_taxonomy_lca(kaiju_taxonomy *t, const uint64_t *ids, uint32_t n);
/* E-value gate + LCA + C/U decision for a batch.  len1/len2 are the nucleotide
   lengths (query_len = len1/3.0 [+ len2/3.0], ConsumerThread.cpp:698,704); pass
   off as given to classify_batch.  db_length from kaiju_gpu_index_get_info. */
/* ---- verbose output: columns 6 and 7 of kaiju -v ------------------------- */
/* ConsumerThread.cpp:527-536 (Greedy), :614-623 (MEM), :820-824 (accessions).  Per read: the
   sequences whose names give the accession set of column 6 (first 20 distinct ones in the order the
   reference visits the rows; the caller prints the sorted set of kaiju_gpu_index_seq_name() prefixes
   up to the last '_') and the text of column 7 ("PEPTIDE,PEPTIDE,").  The search kernels of the
   default path in instantiations that note where every match lies in its read (MEM: k_mem_vb /
   k_mem_wide2_vb) or keep, per best match, its place and the substitutions of its variant (Greedy:
   k_greedy2_vb / k_greedy2_wide_vb), and a pass over the records in front of the locate
   (k_mem_verbose).  Reads that take the retry pass or the exact pass: first-generation kernels. */
#define KAIJU_GPU_MAX_ACC 20
typedef struct {
  uint32_t n_acc;
  uint32_t text_len;                      /* bytes at text + r * text_stride, 0-terminated (packed: at *text + text_pos[r]) */
  uint32_t truncated;                     /* the peptides did not fit */
  uint32_t acc_iseq[KAIJU_GPU_MAX_ACC];
} kaiju_gpu_verbose;
int kaiju_gpu_classify_batch_verbose(kaiju_gpu_ctx *ctx, const char *seqs, const uint64_t *off, uint32_t n_reads,
                                     int paired, kaiju_gpu_hit *out, kaiju_gpu_verbose *vout, char *text,
                                     uint32_t text_stride);
/* The same with column 7 of the whole batch as ONE string owned by the context: read r's text is
   (*text)[text_pos[r] .. text_pos[r] + vout[r].text_len), not terminated; *text_bytes = the length of
   the string.  *text stays valid until the next verbose call on this context (or its destruction).
   No row of text_stride bytes per read to allocate and walk: what the command line programs call. */
int kaiju_gpu_classify_batch_verbose_packed(kaiju_gpu_ctx *ctx, const char *seqs, const uint64_t *off, uint32_t n_reads,
                                            int paired, kaiju_gpu_hit *out, kaiju_gpu_verbose *vout, uint64_t *text_pos,
                                            const char **text, uint64_t *text_bytes);
/* text_stride that holds column 7 of every read of a batch whose longest read (both mates of a pair together) has
   max_pair_len letters: callers size `text` with it instead of guessing the library's bound */
uint32_t kaiju_gpu_verbose_text_stride(uint32_t max_pair_len, int input_is_protein);
/* name of database sequence iseq as stored in the .fmi ("accession_taxid"), NULL if out of range */
const char *kaiju_gpu_index_seq_name(const kaiju_gpu_index *index, uint32_t iseq);

/* ---- LCA on the device: 16-byte records instead of 184-byte ones ------- */
/* (what crosses PCIe / xGMI when the matched ids themselves are not needed, i.e. without -v;
   SURVEY.md 8f-3.  lca_from_ids util.cpp:194-263 on a device copy of the tree.) */
typedef struct kaiju_gpu_taxonomy kaiju_gpu_taxonomy;
typedef struct {
  uint64_t lca;        /* LCA of the ids of the hit; 0 = no hit, or none of its ids is in nodes.dmp */
  uint32_t best;       /* as kaiju_gpu_hit.best                                                    */
  uint32_t info;       /* kaiju_gpu_hit.flags << 8 | n_ids; bit 31 = KAIJU_HIT_INEXACT               */
} kaiju_gpu_compact;
int kaiju_gpu_taxonomy_upload(const kaiju_taxonomy *t, int device_id, kaiju_gpu_taxonomy **out);
void kaiju_gpu_taxonomy_free(kaiju_gpu_taxonomy *t);
/* d_hits: n records written by kaiju_gpu_classify_batch_device; asynchronous on stream (NULL = the context's own
   stream, i.e. behind a classify_batch_device call that was also given NULL) */
int kaiju_gpu_lca_batch_device(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const kaiju_gpu_hit *d_hits,
                               uint32_t n_reads, kaiju_gpu_compact *d_out, void *stream);
/* kaiju_gpu_classify_batch_device + kaiju_gpu_lca_batch_device in ONE call (round 6): where the configuration allows - MEM on an
   index below 2^32 rows with its row -> taxon table - the search's post-search pass writes the 16-byte records itself instead
   of a pass of its own over the 184-byte ones; everywhere else this is the two calls.  d_hits (n records) is the search's working
   set here, not an output: behind the call best / n_ids / flags and the first n_ids ids of every record are what
   kaiju_gpu_classify_batch_device writes, the id slots behind them are unspecified (not zeroed: 1.84 GB less to write per
   10 M reads).  What the reference does at this point: ids_from_SI + lca_from_ids per read in its
   ConsumerThread (src/ConsumerThread.cpp:591-612, src/util.cpp:194-263) */
int kaiju_gpu_classify_batch_device_compact(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const void *d_seqs, uint64_t seq_bytes,
                                            const uint64_t *d_off, uint32_t n_reads, int paired,
                                            kaiju_gpu_hit *d_hits, kaiju_gpu_compact *d_out, void *stream);
/* kaiju_gpu_classify_batch followed by the LCA on the device: host buffers in, 16-byte records out */
int kaiju_gpu_classify_batch_compact(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const char *seqs,
                                     const uint64_t *off, uint32_t n_reads, int paired, kaiju_gpu_compact *out);
/* LCA of host hit records through the device (blocking) */
int kaiju_gpu_lca_batch(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const kaiju_gpu_hit *hits,
                        uint32_t n_reads, kaiju_gpu_compact *out);
/* kaiju_finalize_hits for compact records (E-value gate, C/U decision; the LCA is already in them) */
int kaiju_finalize_compact(const kaiju_gpu_params *p, double db_length, const kaiju_gpu_compact *recs,
                           const uint64_t *off, uint32_t n_reads, int paired, kaiju_result *out);

/* ---- record extraction on the device: FASTQ / FASTA text in, seqs / off out ------------------------------ */
/* What the reference does in its reading loop (kaiju.cpp:288-386) and the command line programs here do on the host
   (BlockCursor in csrc/host/kaiju_main.cpp), as HIP passes (kaiju_amd/csrc/ingest.hip; the rules: kj_ingest.h).  A text is a
   block of WHOLE records below 2^32 bytes.  Format and keep_names (kaijup: the name is the whole header line without its
   first byte) are arguments, nothing is detected.  Out come the buffers of kaiju_gpu_classify_batch_device[_compact]: seqs,
   the strip()'d letters, and off[2n + 1]; with a second text record r of text 2 is the mate of record r of text 1 and
   n = min(n_records, n_records2) reads are emitted (the records of the longer text's tail are counted only).  names[r] is
   where the name of record r lies in text 1. */
typedef struct kaiju_gpu_name_span { uint32_t pos, len; } kaiju_gpu_name_span;
typedef struct kaiju_gpu_parse_info {
  uint32_t n_records, n_records2;  /* records found in text 1 / text 2 (0 when unpaired)                                   */
  uint32_t max_mate_len;           /* longest stripped mate emitted: what kaiju_gpu_set_max_read_length wants              */
  uint32_t name_mismatch;          /* first emitted record whose names differ between the texts, ~0u: none                 */
  uint64_t seq_bytes;              /* bytes written to seqs = off[2 * reads emitted]                                       */
  uint32_t overflow, reserved;     /* 1: more reads than rec_cap; the first rec_cap are emitted, nothing behind the         */
                                   /* capacities is written                                                                */
} kaiju_gpu_parse_info;
/* All pointers are device pointers on the context's GPU; the text pointers must be 16-byte aligned (KAIJU_GPU_ERR_ARG
   otherwise).  d_text2 = NULL, bytes2 = 0: unpaired.  Asynchronous on `stream` (NULL: the context's own).  The scratch - a line
   table sized for the worst case, a text of nothing but '\n': 5 bytes per byte of text - lives in the context and grows
   when a call needs more. */
int kaiju_gpu_parse_block_device(kaiju_gpu_ctx *ctx, const void *d_text1, uint64_t bytes1, const void *d_text2, uint64_t bytes2,
                                 int fastq, int keep_names, uint32_t rec_cap, void *d_seqs /* >= bytes1 + bytes2 */,
                                 uint64_t *d_off /* 2 * rec_cap + 1 */, kaiju_gpu_name_span *d_names /* rec_cap */,
                                 kaiju_gpu_parse_info *d_info, void *stream);
/* The same with host pointers (text up, results down); blocks. */
int kaiju_gpu_parse_block(kaiju_gpu_ctx *ctx, const char *text1, uint64_t bytes1, const char *text2, uint64_t bytes2, int fastq,
                          int keep_names, uint32_t rec_cap, char *seqs, uint64_t *off, kaiju_gpu_name_span *names,
                          kaiju_gpu_parse_info *info);
/* Text in, 16-byte records out: upload, the passes above, one read-back of *info, kaiju_gpu_set_max_read_length(
   info->max_mate_len) and kaiju_gpu_classify_batch_device_compact on the same stream; out (n records), off (2n + 1: what
   kaiju_finalize_compact wants) and names (n) come back.  info->overflow: KAIJU_GPU_ERR_ARG, nothing classified.  A name
   mismatch or a shorter second text is reported in *info and left to the caller. */
int kaiju_gpu_classify_text_compact(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const char *text1, uint64_t bytes1,
                                    const char *text2, uint64_t bytes2, int fastq, int keep_names, uint32_t rec_cap,
                                    kaiju_gpu_compact *out, uint64_t *off, kaiju_gpu_name_span *names,
                                    kaiju_gpu_parse_info *info);

/* ---- the output lines on the device: 16-byte records in, text out ----------------------------------------- */
/* What stage 4 of the command line programs does on the host for kaiju / kaiju-multi without -v, as HIP passes
   (kaiju_amd/csrc/format.hip; the rules: kj_format.h): per record the decision of kaiju_finalize_compact (E-value gate
   included, bit for bit: the table argument is in kj_format.h) and the line "C\t<name>\t<taxon>\n" or "U\t<name>\t0\n", the
   name being text1[names[r].pos, + names[r].len); the lines of records 0 .. n - 1 follow each other in `out`.  Mode,
   use_evalue, min_evalue and input_is_protein are the context's, db_length its index's.  The lines of -v are made by the passes of
   kaiju_gpu_format_verbose, those of kaijux and kaijup by the passes of kaiju_gpu_format_seq, both further down. */
typedef struct kaiju_gpu_format_info {
  uint64_t text_bytes;             /* size of the whole text, whether or not it fitted                                      */
  uint32_t n_records, n_classified;/* records formatted (= n), 'C' lines among them                                         */
  uint32_t overflow;               /* 1: text_bytes > out_cap; the whole lines that fit are written, no byte at or behind   */
                                   /* out_cap is touched                                                                    */
  uint32_t n_inexact;              /* (the reserved word) records whose info carries KAIJU_HIT_INEXACT: they are formatted   */
                                   /* like any other, a caller that must not print such lines looks here                    */
} kaiju_gpu_format_info;
/* All pointers are device pointers on the context's GPU; d_out must be 16-byte aligned (KAIJU_GPU_ERR_ARG otherwise), text 1
   below 2^32 - 32 bytes.  d_recs: n records, d_off: 2n + 1 (as given to the classification), d_names: n.  Asynchronous on
   `stream` (NULL: the context's own); nothing waits for the host.  The scratch - 20 bytes per record - lives in the context
   and grows when a call needs more. */
int kaiju_gpu_format_compact_device(kaiju_gpu_ctx *ctx, const kaiju_gpu_compact *d_recs, const uint64_t *d_off, uint32_t n, int paired,
                                    const void *d_text1, uint64_t bytes1, const kaiju_gpu_name_span *d_names, void *d_out,
                                    uint64_t out_cap, kaiju_gpu_format_info *d_info, void *stream);
/* The same with host pointers (records, text and names up; *info and the bytes written down); blocks.  out[0 .. out_cap):
   only the bytes of the lines written change. */
int kaiju_gpu_format_compact(kaiju_gpu_ctx *ctx, const kaiju_gpu_compact *recs, const uint64_t *off, uint32_t n, int paired,
                             const char *text1, uint64_t bytes1, const kaiju_gpu_name_span *names, char *out, uint64_t out_cap,
                             kaiju_gpu_format_info *info);
/* Host only: an out_cap that cannot overflow for n records whose names are disjoint pieces of a text of bytes1 bytes
   (a line is its name and at most 24 bytes more): bytes1 + 24 * n */
uint64_t kaiju_gpu_format_bound(uint64_t bytes1, uint32_t n);
/* Host only: the table of the E-value gate as the library builds it for its contexts, pow(2, -bitscore(best)) for best <
   n_out (at most 4096 entries are written).  Returns 0, or KAIJU_GPU_ERR_UNSUPPORTED when a score beyond the table has a
   factor other than +0.0 on this host (the format entry points refuse to run then). */
int kaiju_gpu_format_evalue_table(double *out, uint32_t n_out);
/* Text in, text out: upload, the passes of kaiju_gpu_classify_text_compact and the passes above on one stream; what comes back
   is *info_parse (read back in front of the classification, as there), *info_format and exactly info_format->text_bytes bytes
   of out_text.  The stops of kaiju_gpu_classify_text_compact stay: info_parse->overflow is KAIJU_GPU_ERR_ARG with nothing
   classified, a name mismatch or a shorter second text is reported in *info_parse and left to the caller.  out_cap below
   the text's size (kaiju_gpu_format_bound(bytes1, rec_cap) never is): KAIJU_GPU_ERR_ARG, *info_format says what is needed. */
int kaiju_gpu_classify_text_to_text(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const char *text1, uint64_t bytes1,
                                    const char *text2, uint64_t bytes2, int fastq, int keep_names, uint32_t rec_cap,
                                    char *out_text, uint64_t out_cap, kaiju_gpu_parse_info *info_parse,
                                    kaiju_gpu_format_info *info_format);

/* ---- taxon names and lineages in the output lines: the column of kaiju-addTaxonNames ------------------------ */
/* What kaiju-addTaxonNames (kaiju-addTaxonNames.cpp, util.cpp:123-192 of the reference) appends to the 'C' lines, written by
   the passes that write the lines (kaiju_amd/csrc/format_names.hip; the rules: kj_format_names.h).  A 'C' line whose taxon is
   no node of nodes.dmp as that tool parses it, or has no scientific name of its own, stays as it is; every other 'C' line
   gets "\t" and the taxon's name (KAIJU_NAMES_NAME), its lineage root first, every name followed by "; " (KAIJU_NAMES_PATH, the
   tool's -p), or the names at the ranks of a comma separated list, "NA" where the lineage has none (KAIJU_NAMES_RANKS, -r).
   A tree with a cycle other than a node that is its own parent is refused (KAIJU_GPU_ERR_ARG; kaiju_gpu_last_error() names
   a node on it), so is a list of more than KAIJU_NAMES_MAX_RANKS distinct ranks or KAIJU_NAMES_MAX_LIST items. */
#define KAIJU_NAMES_NAME 0
#define KAIJU_NAMES_PATH 1
#define KAIJU_NAMES_RANKS 2
#define KAIJU_NAMES_MAX_RANKS 16
#define KAIJU_NAMES_MAX_LIST 64
typedef struct kaiju_taxon_names kaiju_taxon_names;           /* host tables */
typedef struct kaiju_gpu_taxon_names kaiju_gpu_taxon_names;   /* ... on a device, with the tables built there */
/* Host only, no GPU.  ranks_csv: the list of KAIJU_NAMES_RANKS (NULL or ignored otherwise) */
int kaiju_taxon_names_load(const char *nodes_dmp, const char *names_dmp, int mode, const char *ranks_csv, kaiju_taxon_names **out);
void kaiju_taxon_names_free(kaiju_taxon_names *names);
/* Host only, for inspection: the annotation of `taxon`, computed by walking the tree (not from the tables the device uses).
   Returns its length - the first min(length, cap) bytes are in buf - or -1: the line stays unchanged */
int64_t kaiju_taxon_names_annotation(const kaiju_taxon_names *names, uint64_t taxon, char *buf, uint64_t cap);
/* nodes of the tree / nodes with a name of their own */
uint64_t kaiju_taxon_names_count(const kaiju_taxon_names *names, int named);
/* Upload, and the per-slot tables built by kernels there (lengths of the lineages; per rank the node that supplies it).
   KAIJU_GPU_ERR_ARG when an annotation reaches 2^24 bytes */
int kaiju_gpu_taxon_names_upload(const kaiju_taxon_names *names, int device_id, kaiju_gpu_taxon_names **out);
void kaiju_gpu_taxon_names_free(kaiju_gpu_taxon_names *names);
uint64_t kaiju_gpu_taxon_names_max_annotation(const kaiju_gpu_taxon_names *names);
/* For inspection: the tables as they lie on the device, to the host.  which: 0 key (8 bytes per slot), 1 parent, 2 name_pos,
   3 name_len, 4 path_len, 5 rank_len (4 each), 6 rank_src (4 * distinct ranks), 7 rank (1).  A table the mode does not build:
   KAIJU_GPU_ERR_ARG.  *n_slots (may be NULL): slots of the table */
int kaiju_gpu_taxon_names_read(const kaiju_gpu_taxon_names *names, int which, void *host_out, uint64_t out_bytes, uint64_t *n_slots);
typedef struct kaiju_gpu_format_names_info {
  uint64_t text_bytes;             /* the fields of kaiju_gpu_format_info, with the same meaning                            */
  uint32_t n_records, n_classified;
  uint32_t overflow;
  uint32_t n_inexact;
  uint32_t n_unknown_taxon;        /* 'C' lines left unchanged: the taxon is no node of the tree                           */
  uint32_t n_unnamed_taxon;        /* 'C' lines left unchanged: the taxon has no name                                      */
  uint32_t n_dropped;              /* 'U' lines left out (drop_unclassified)                                               */
  uint32_t reserved;
} kaiju_gpu_format_names_info;     /* 40 bytes */
/* kaiju_gpu_format_compact_device / kaiju_gpu_format_compact with the column.  `names` must live on the context's device.
   drop_unclassified: the tool's -u.  Lines are written whole or not at all, no byte at or behind out_cap is touched.
   The scratch - 24 bytes per record - lives in the context. */
int kaiju_gpu_format_names_device(kaiju_gpu_ctx *ctx, const kaiju_gpu_compact *d_recs, const uint64_t *d_off, uint32_t n, int paired,
                                  const void *d_text1, uint64_t bytes1, const kaiju_gpu_name_span *d_names,
                                  const kaiju_gpu_taxon_names *names, int drop_unclassified, void *d_out, uint64_t out_cap,
                                  kaiju_gpu_format_names_info *d_info, void *stream);
int kaiju_gpu_format_names(kaiju_gpu_ctx *ctx, const kaiju_gpu_compact *recs, const uint64_t *off, uint32_t n, int paired,
                           const char *text1, uint64_t bytes1, const kaiju_gpu_name_span *names_spans,
                           const kaiju_gpu_taxon_names *names, int drop_unclassified, char *out, uint64_t out_cap,
                           kaiju_gpu_format_names_info *info);
/* Host only: an out_cap that cannot overflow: bytes1 + n * (25 + max_annotation) */
uint64_t kaiju_gpu_format_names_bound(uint64_t bytes1, uint32_t n, const kaiju_gpu_taxon_names *names);
/* kaiju_gpu_classify_text_to_text with the passes above at its end */
int kaiju_gpu_classify_text_to_text_names(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const char *text1, uint64_t bytes1,
                                          const char *text2, uint64_t bytes2, int fastq, int keep_names, uint32_t rec_cap,
                                          const kaiju_gpu_taxon_names *names, int drop_unclassified, char *out_text, uint64_t out_cap,
                                          kaiju_gpu_parse_info *info_parse, kaiju_gpu_format_names_info *info_format);

/* ---- kaiju-addTaxonNames on existing output text: lines in, annotated lines out ------------------------------- */
/* The column above for lines that exist already - an earlier run's, those of kaiju -v, kaijux / kaijup, the reference's own
   kaiju (kaiju_amd/csrc/annotate.hip; the rules: kj_annotate.h, those of kaiju-addTaxonNames.cpp:133-228):
     - a line ends at '\n'; the last one may lack it and gets one; a line of length 0 gives nothing; every other byte, '\r' and
       NUL included, is a byte of the line
     - byte 0 is not 'C': the line is copied unchanged, or left out with drop_unclassified (the tool's -u)
     - a 'C' line: the id is the run of [0-9] directly behind the second tab, whatever follows it ("7abc", "7\t..." read 7).
       Fewer than two tabs, an empty run, a value above 2^64 - 1 (by value), an id that is no node, a node without a name of
       its own: the line is copied unchanged, also under drop_unclassified
     - else: line "\t" annotation "\n", the annotation that of kaiju_gpu_format_names in the mode of `names`
   The annotator is scratch on the device of `names`; it needs no index and no context.  One call at a time per annotator. */
typedef struct kaiju_gpu_annotator kaiju_gpu_annotator;
int kaiju_gpu_annotator_create(const kaiju_gpu_taxon_names *names, kaiju_gpu_annotator **out);
void kaiju_gpu_annotator_free(kaiju_gpu_annotator *a);
typedef struct kaiju_gpu_annotate_info {
  uint64_t text_bytes;             /* size of the whole annotated text, also when it overflowed                            */
  uint32_t n_lines;                /* lines of the input, those of length 0 included                                       */
  uint32_t n_c_lines;              /* lines whose byte 0 is 'C'                                                            */
  uint32_t n_annotated;            /* ... that got the column                                                              */
  uint32_t n_bad_id;               /* ... without a readable id: fewer than two tabs, no digit, above 2^64 - 1             */
  uint32_t n_unknown_taxon;        /* ... whose id is no node of the tree                                                  */
  uint32_t n_unnamed_taxon;        /* ... whose node has no name                                                           */
  uint32_t n_dropped;              /* other lines left out (drop_unclassified)                                             */
  uint32_t n_empty;                /* lines of length 0                                                                    */
  uint32_t overflow;
  uint32_t reserved;
} kaiju_gpu_annotate_info;         /* 48 bytes */
/* All pointers device pointers; every pass is queued on `stream` and nothing synchronises, so d_text may be the d_out of
   kaiju_gpu_format_verbose_device / _seq_device / _compact_device queued on the same stream in front of it.  d_text and d_out
   are 16-byte aligned and d_text is readable up to the next multiple of 16 behind bytes (KAIJU_GPU_ERR_ARG otherwise, as for
   bytes above 2^32 - 16).  bytes == 0 writes nothing.  Lines are written whole or not at all, no byte at or behind out_cap is
   touched.  The scratch - 24 bytes per byte of text, sized for a text of nothing but '\n' - lives in the annotator. */
int kaiju_gpu_annotate_text_device(kaiju_gpu_annotator *a, const void *d_text, uint64_t bytes, int drop_unclassified,
                                   void *d_out, uint64_t out_cap, kaiju_gpu_annotate_info *d_info, void *stream);
/* The same for host memory (no alignment asked for): upload, the passes, the download of the lines written */
int kaiju_gpu_annotate_text(kaiju_gpu_annotator *a, const char *text, uint64_t bytes, int drop_unclassified,
                            char *out, uint64_t out_cap, kaiju_gpu_annotate_info *info);
/* Host only: an out_cap that cannot overflow for a text of n_lines lines (its '\n' bytes plus one):
   bytes + 1 + n_lines * (1 + max_annotation) */
uint64_t kaiju_gpu_annotate_bound(uint64_t bytes, uint64_t n_lines, const kaiju_gpu_taxon_names *names);

/* ---- kaiju-mergeOutputs on two output texts: lines of two runs in, merged lines out --------------------------- */
/* Line k of text 1 and line k of text 2 - two classifications of the same reads, sorted alike - give line k of the output
   (kaiju_amd/csrc/merge.hip; the rules: kj_merge.h, those of kaiju-mergeOutputs.cpp:110-295, :355-399 and util.cpp:42-77):
     - U,U: "U\t<name>\t0\n".  C,U / U,C: "C\t<name>\t<id>[\t<score>]\n" of the classified side.  C,C: equal id texts give id1
       and the score text of the larger value; different score values give the id and score of the larger one; else score1
       and, by `conflict`, id1, id2, the tool's own LCA printed as a number, or the lower of the two in one lineage
     - with use_score (the tool's -s) a 'C' line needs a fourth column; the id is then every byte of the third
     - the first pair that fails (KAIJU_GPU_MERGE_STOP_*) ends the run: the pairs in front of it are written, nothing else
     - scores are compared as decimals.  A C,C pair with a score of more than 15 significant digits, or outside
       [1e-300, 1e300) and below 1e309, stops the run with KAIJU_GPU_MERGE_STOP_SCORE_WIDE rather than guess what the
       comparison of the doubles would give
   The merger is scratch on the device of `tax`; it needs no index and no context.  One call at a time per merger. */
enum { KAIJU_GPU_MERGE_FIRST = 0, KAIJU_GPU_MERGE_SECOND = 1, KAIJU_GPU_MERGE_LCA = 2, KAIJU_GPU_MERGE_LOWEST = 3 };   /* -c 1, 2, lca, lowest */
enum {
  KAIJU_GPU_MERGE_STOP_NONE = 0,
  KAIJU_GPU_MERGE_STOP_1_CLASS = 1,    /* line of text 1: byte 0 is neither 'C' nor 'U' (an empty line too)                */
  KAIJU_GPU_MERGE_STOP_1_TABS = 2,     /* ... fewer than two tabs                                                          */
  KAIJU_GPU_MERGE_STOP_1_COLUMN = 3,   /* ... nothing behind tab 2; with use_score on a 'C' line: no tab 3, nothing behind it */
  KAIJU_GPU_MERGE_STOP_2_SHORT = 4,    /* text 2 has no such line (final only)                                             */
  KAIJU_GPU_MERGE_STOP_2_CLASS = 5,    /* the three above for the line of text 2                                           */
  KAIJU_GPU_MERGE_STOP_2_TABS = 6,
  KAIJU_GPU_MERGE_STOP_2_COLUMN = 7,
  KAIJU_GPU_MERGE_STOP_NAMES = 8,      /* the names differ                                                                 */
  KAIJU_GPU_MERGE_STOP_SCORE_WIDE = 9  /* a score outside what the device compares exactly                                 */
};
typedef struct kaiju_gpu_merger kaiju_gpu_merger;
/* tax == NULL: the empty tree (device_id says where the merger lives; with a tree it must be the tree's device).
   KAIJU_GPU_MERGE_LCA without a tree is KAIJU_GPU_ERR_ARG, as the tool refuses -c lca without -t */
int kaiju_gpu_merger_create(const kaiju_gpu_taxonomy *tax, int device_id, int conflict, int use_score, kaiju_gpu_merger **out);
void kaiju_gpu_merger_free(kaiju_gpu_merger *m);
typedef struct kaiju_gpu_merge_info {
  uint64_t text_bytes;             /* size of the whole merged text, also when it overflowed                               */
  uint64_t used1, used2;           /* bytes of text 1 / 2 in the lines that were paired; the caller carries the rest       */
  uint64_t n_pairs;                /* the smaller of the two line counts                                                   */
  uint64_t count;                  /* lines of text 1 read: the pairs written and the one that stopped (the tool's -v)     */
  uint64_t count_c1, count_c2;     /* written pairs classified in text 1 / in text 2                                       */
  uint64_t count_c12, count_c3;    /* ... in both / in either                                                              */
  uint64_t count_c1_not_c2, count_c2_not_c1;
  uint64_t stop_pair;              /* index of the pair that stopped the run; all ones: none                               */
  uint32_t stop_why;               /* KAIJU_GPU_MERGE_STOP_*                                                               */
  uint32_t more_in_2;              /* final, no stop: text 2 has a further line and it is not empty (the tool warns)       */
  uint32_t overflow;
  uint32_t reserved;
} kaiju_gpu_merge_info;            /* 112 bytes */
/* All pointers device pointers; every pass is queued on `stream` and nothing synchronises, so d_text1 / d_text2 may be the
   d_out of two formatter calls queued on the same stream in front of it.  The three buffers are 16-byte aligned and the texts
   readable up to the next multiple of 16 behind their bytes (KAIJU_GPU_ERR_ARG otherwise, as for bytes of 2^32 - 16 and more
   and for buffers on another device).  final == 0: only lines a '\n' ends count, n_pairs of them are merged and used1 / used2
   say where the rest starts.  final != 0: a last line without '\n' is a line, more lines in text 1 stop the run, more in text 2
   set more_in_2.  Lines are written whole or not at all, no byte at or behind out_cap is touched.  The scratch - 4 bytes per
   byte of either text and 12 per byte of the shorter one - lives in the merger. */
int kaiju_gpu_merge_text_device(kaiju_gpu_merger *m, const void *d_text1, uint64_t bytes1, const void *d_text2, uint64_t bytes2,
                                int final, void *d_out, uint64_t out_cap, kaiju_gpu_merge_info *d_info, void *stream);
/* The same for host memory (no alignment asked for): upload, the passes, the download of the lines written */
int kaiju_gpu_merge_text(kaiju_gpu_merger *m, const char *text1, uint64_t bytes1, const char *text2, uint64_t bytes2, int final,
                         char *out, uint64_t out_cap, kaiju_gpu_merge_info *info);
/* Host only: an out_cap that cannot overflow: bytes1 + bytes2 + 2 + 20 * (min(bytes1, bytes2) / 4 + 2) */
uint64_t kaiju_gpu_merge_bound(uint64_t bytes1, uint64_t bytes2);
/* Diagnostics.  A merger created with KAIJU_GPU_MERGE_TIMES=1 in the environment records a HIP event between the passes of
   every call (KAIJU_GPU_ERR_UNSUPPORTED otherwise): the milliseconds of the last call's passes - lines and plan, pair, count,
   offsets, write, finish - into ms[0 .. n), n <= KAIJU_GPU_MERGE_PASSES.  Waits for that call. */
enum { KAIJU_GPU_MERGE_PASSES = 6 };
int kaiju_gpu_merge_pass_ms(kaiju_gpu_merger *m, float *ms, uint32_t n);

/* ---- kaiju2table on output texts: lines in, reads per taxon out ------------------------------------------------ */
/* What kaiju2table.cpp:192-236 keeps per input file, kept per slot of the tree of `names` on its device
   (kaiju_amd/csrc/tally.hip; the rules: kj_tally.h):
     - every line that is not empty counts in n_total; byte 0 not 'C': n_unclassified
     - the id is the run of digits behind the second tab.  None, or a value above 2^64 - 1: n_bad_id.  No node of nodes.dmp:
       n_unknown_taxon.  Else the node's direct count rises, and n_virus when the node is 10239 or below it
     - at kaiju_gpu_tally_result a node's reads count for itself and for every ancestor but a node that is its own parent;
       those of a node at or below 10239 count for that node alone
   Texts are added in as many calls as the caller likes; nothing reaches the host before kaiju_gpu_tally_result.  `names` may
   be of any mode (only its keys and parents are read) and must outlive the tally.  One call at a time per tally; calls on
   different streams are ordered by an event of the tally. */
typedef struct kaiju_gpu_tally kaiju_gpu_tally;
int kaiju_gpu_tally_create(const kaiju_gpu_taxon_names *names, kaiju_gpu_tally **out);
void kaiju_gpu_tally_free(kaiju_gpu_tally *t);
/* every count back to 0 (a new input file) */
int kaiju_gpu_tally_reset(kaiju_gpu_tally *t);
typedef struct kaiju_gpu_tally_info {
  uint64_t used;                   /* bytes of the text in the lines that were counted; the caller carries the rest        */
  uint64_t n_lines;                /* lines looked at, empty ones included                                                 */
  uint64_t n_total, n_unclassified, n_bad_id, n_unknown_taxon, n_virus;
} kaiju_gpu_tally_info;            /* 56 bytes */
/* All pointers device pointers; every pass is queued on `stream` and nothing synchronises, so d_text may be the d_out of a
   formatter call queued on the same stream in front of it.  d_text is 16-byte aligned and readable up to the next multiple
   of 16 behind its bytes (KAIJU_GPU_ERR_ARG otherwise, as for bytes of 2^32 - 16 and more and for a buffer on another device).
   final == 0: only lines a '\n' ends count and `used` says where the rest starts.  final != 0: a last line without '\n' is
   a line.  *d_info describes this call alone.  The scratch - 4 bytes per byte of the text - lives in the tally. */
int kaiju_gpu_tally_add_text_device(kaiju_gpu_tally *t, const void *d_text, uint64_t bytes, int final, kaiju_gpu_tally_info *d_info,
                                    void *stream);
/* The same for host memory (no alignment asked for): upload, the passes, the info */
int kaiju_gpu_tally_add_text(kaiju_gpu_tally *t, const char *text, uint64_t bytes, int final, kaiju_gpu_tally_info *info);
typedef struct kaiju_gpu_tally_entry {
  uint64_t taxon, direct, summed;  /* reads of the node itself / of what counts for it (> 0)                               */
  uint32_t virus, reserved;        /* 1: the node is 10239 or below it                                                     */
} kaiju_gpu_tally_entry;           /* 32 bytes */
/* Everything since the last reset: the nodes with summed > 0 in a fixed order (that of their slots) into entries[0 .. cap),
   their number into *n_entries, the sums of the infos into *totals (`used`: the sum too).  More than cap nodes:
   KAIJU_GPU_ERR_ARG with *n_entries set and no entry written.  Waits for the calls before it; the counts stay. */
int kaiju_gpu_tally_result(kaiju_gpu_tally *t, kaiju_gpu_tally_entry *entries, uint64_t cap, uint64_t *n_entries, kaiju_gpu_tally_info *totals);
/* Diagnostics.  A tally created with KAIJU_GPU_TALLY_TIMES=1 in the environment records a HIP event between the passes of
   every add call (KAIJU_GPU_ERR_UNSUPPORTED otherwise): the milliseconds of the last call's passes - lines, count, finish -
   into ms[0 .. n), n <= KAIJU_GPU_TALLY_PASSES.  Waits for that call. */
enum { KAIJU_GPU_TALLY_PASSES = 3 };
int kaiju_gpu_tally_pass_ms(kaiju_gpu_tally *t, float *ms, uint32_t n);

/* ---- kaiju2krona on the counts of tallies: one lineage line per taxon -------------------------------------------- */
/* What kaiju2krona.cpp:150-190 writes from its counts, written on the device from the direct counts that tallies hold there
   (kaiju_amd/csrc/krona.hip; the rules: kj_krona.h): for every node with reads and a name of its own the line
   "<reads>\t<name>\t<name>...\n", the lineage root first.  The taxon's own name is printed when its parent's id has a name; an
   ancestor without a name is left out; a parent id that is no node but has a name in names.dmp is printed in front (without a
   list of ranks only).  ranks_csv (the tool's -l; NULL: none): items between commas, empty ones dropped; only names of nodes
   whose rank string is an item are printed, "no rank" being a rank like any other.  The lines are in ascending slot order -
   that of kaiju_gpu_tally_result; the tool's order is that of a hash map - and "<n>\tUnclassified\n" is the last one.
   `names` may be of any mode and must outlive the object; its lineage tables (1 + 1 + 4 bytes per slot, and the names of
   parent ids that are no nodes) are built at create.  KAIJU_GPU_ERR_ARG for a list of more than KAIJU_NAMES_MAX_LIST items
   and for a lineage of 2^24 bytes or more. */
typedef struct kaiju_gpu_krona kaiju_gpu_krona;
enum { KAIJU_GPU_KRONA_MAX_TALLIES = 4 };
int kaiju_gpu_krona_create(const kaiju_gpu_taxon_names *names, const char *ranks_csv, kaiju_gpu_krona **out);
void kaiju_gpu_krona_free(kaiju_gpu_krona *k);
typedef struct kaiju_gpu_krona_info {
  uint64_t text_bytes;             /* of the whole text, also when it overflowed: a call with out_cap == 0 sizes the buffer  */
  uint64_t written_bytes;          /* of the lines that were written                                                       */
  uint64_t n_lines, n_written;     /* lines of the whole text / written                                                    */
  uint64_t n_unnamed_taxa;         /* nodes with reads and no name of their own: no line ...                               */
  uint64_t n_unnamed_reads;        /* ... and their reads                                                                  */
  uint64_t n_unclassified;         /* the count of the Unclassified line (0: no such line)                                 */
  uint32_t overflow, reserved;     /* 1: the text is longer than out_cap; only whole lines in front of out_cap were written */
} kaiju_gpu_krona_info;            /* 64 bytes */
/* The text of the counts of tallies[0 .. n_tallies) (1 .. KAIJU_GPU_KRONA_MAX_TALLIES of them, all on the names of `k`; their
   counts are added per slot and stay as they are).  count_unclassified != 0 (the tool's -u): the Unclassified line, if any
   line was unclassified.  All pointers device pointers; the call waits on the events of the tallies, every pass is queued on
   `stream` (NULL: a stream of the object) and nothing synchronises.  d_out is 16-byte aligned.  A line is written whole or
   not at all and no byte at or behind out_cap is touched.  One call at a time per object.  KAIJU_GPU_ERR_ARG for a tally of
   other names or another device, for 0 or too many tallies and for a misaligned d_out. */
int kaiju_gpu_krona_text_device(kaiju_gpu_krona *k, kaiju_gpu_tally *const *tallies, uint32_t n_tallies, int count_unclassified, void *d_out,
                                uint64_t out_cap, kaiju_gpu_krona_info *d_info, void *stream);
/* The same into host memory; blocks.  cap == 0 with buf == NULL: only the info */
int kaiju_gpu_krona_text(kaiju_gpu_krona *k, kaiju_gpu_tally *const *tallies, uint32_t n_tallies, int count_unclassified, char *buf, uint64_t cap,
                         kaiju_gpu_krona_info *info);
/* Diagnostics.  An object created with KAIJU_GPU_KRONA_TIMES=1 in the environment records a HIP event between the passes of
   every call (KAIJU_GPU_ERR_UNSUPPORTED otherwise): the milliseconds of the last call's passes - select, compact, len and
   offsets, write, finish - into ms[0 .. n), n <= KAIJU_GPU_KRONA_PASSES.  Waits for that call. */
enum { KAIJU_GPU_KRONA_PASSES = 5 };
int kaiju_gpu_krona_pass_ms(kaiju_gpu_krona *k, float *ms, uint32_t n);

/* ---- kaiju-convertNR: the accession map and the conversion of nr-style text ------------------------------------- */
/* The accession -> taxon map of kaiju-convertNR.cpp:145-194, built and probed on the device (kaiju_amd/csrc/accmap.hip; the
   rules: kj_convert.h): open addressing over 64-bit slots, the keys compacted into an arena of { line number, taxon, length,
   key } entries, ~ 24 + the key rounded up to 8 bytes each.  The first line that inserts a key wins, whatever the order of the
   lanes and however the file is cut into blocks.  Slots (rehash at a load of 1/2) and the arena grow on demand; every
   allocation is checked against the free device memory first (KAIJU_GPU_ERR_NOMEM with both numbers).  Every probe loop is
   bounded by the number of slots: a table that is full all the same is KAIJU_GPU_ERR_FORMAT, never a spin.
   `tax` (it must outlive the map) and merged_pairs - n_merged pairs { old id, new id } of merged.dmp, the first pair of an old id
   wins - decide which lines insert; tax == NULL makes a map for kaiju_gpu_accmap_add_keys only.  key_col / taxon_col: the columns
   (from 0) of key and taxon; 1 and 2, the tool's, is what exists (KAIJU_GPU_ERR_UNSUPPORTED otherwise).  initial_slots is
   rounded up to a power of two, at least 8 (0: 2^16). */
typedef struct kaiju_gpu_accmap kaiju_gpu_accmap;
int kaiju_gpu_accmap_create(const kaiju_gpu_taxonomy *tax, int device_id, const uint64_t *merged_pairs, uint64_t n_merged, uint32_t key_col,
                            uint32_t taxon_col, uint64_t initial_slots, kaiju_gpu_accmap **out);
/* The same with a rule set in place of the columns.  KAIJU_GPU_CONVERT_RULES_NR: what kaiju_gpu_accmap_create (1, 2) makes.
   KAIJU_GPU_CONVERT_RULES_REFSEQ: the map of kaiju-convertRefSeq.cpp:145-195 - two columns accession.version '\t' taxon, only
   lines that begin with "WP_", taxon 0 inserts nothing, and an accession whose taxon came through merged.dmp loses its last
   byte, as in the tool (kj_convert.h, "kaiju-convertRefSeq").  kaiju_gpu_accmap_add_keys, _lookup, _info and the growth are
   the same for both.  Any other value: KAIJU_GPU_ERR_ARG. */
enum { KAIJU_GPU_CONVERT_RULES_NR = 0, KAIJU_GPU_CONVERT_RULES_REFSEQ = 1 };
int kaiju_gpu_accmap_create_rules(const kaiju_gpu_taxonomy *tax, int device_id, const uint64_t *merged_pairs, uint64_t n_merged, int rules,
                                  uint64_t initial_slots, kaiju_gpu_accmap **out);
void kaiju_gpu_accmap_free(kaiju_gpu_accmap *m);
/* A block of the map file, cut behind a line end (the last block need not end in one); is_first_block: its first line is the
   file's header line and is skipped.  Blocks below 2^32 - 16 bytes.  The call blocks.  The _device form takes a 16-byte aligned
   device pointer with 16 readable bytes behind the text. */
int kaiju_gpu_accmap_add_text(kaiju_gpu_accmap *m, const char *text, uint64_t n, int is_first_block);
int kaiju_gpu_accmap_add_text_device(kaiju_gpu_accmap *m, const void *d_text, uint64_t n, int is_first_block);
/* Every non-empty line, whole, is a key with the value `value` (the excluded accessions of -e) */
int kaiju_gpu_accmap_add_keys(kaiju_gpu_accmap *m, const char *text, uint64_t n, uint64_t value);
/* Tests and diagnostics: the taxon of every line of `keys` (an empty line is the key of zero bytes) into taxa[0 .. min(lines, cap)),
   KAIJU_GPU_ACCMAP_MISS for a key the map does not hold; *n_keys: the lines */
#define KAIJU_GPU_ACCMAP_MISS (~0ull)
int kaiju_gpu_accmap_lookup(kaiju_gpu_accmap *m, const char *keys, uint64_t n, uint64_t *taxa, uint64_t cap, uint64_t *n_keys);
typedef struct kaiju_gpu_accmap_stats {
  uint64_t entries;                /* distinct keys                                                                        */
  uint64_t slots;
  uint64_t arena_bytes, arena_cap; /* used (entries that lost a race for their slot included) / allocated                  */
  uint64_t lines;                  /* non-empty lines seen, the header line not counted                                    */
  uint64_t lines_no_insert;        /* ... that inserted nothing: ULONG_MAX, neither node nor merged to one                 */
  uint64_t duplicates;             /* ... whose key another line had inserted                                              */
  uint64_t rehashes;
  uint64_t probe_hist[16];         /* entries by the slots a lookup of their key reads: 1, 2, .. 15, 16 or more            */
  uint64_t reserved[8];
} kaiju_gpu_accmap_stats;          /* 256 bytes */
int kaiju_gpu_accmap_info(kaiju_gpu_accmap *m, kaiju_gpu_accmap_stats *out);
/* With KAIJU_GPU_CONVERT_TIMES=1 at create: the milliseconds of the last add call's passes - lines, parse, grow, insert, resolve */
enum { KAIJU_GPU_ACCMAP_PASSES = 5 };
int kaiju_gpu_accmap_pass_ms(kaiju_gpu_accmap *m, float *ms, uint32_t n);

/* What kaiju-convertNR.cpp:221-306 writes for a block of nr-style text (kaiju_amd/csrc/convert.hip; the rules: kj_convert.h):
   per kept record '>' [first accession with a taxon '_'] taxon '\n' letters '\n', in the order of the text.  The block starts
   at a header line or is the start of the file; the '\n' of a file of which nothing is kept is the caller's.  include_ids: the
   ids of -l that are nodes (NULL with n_include 0: 2, 2157, 10239).  `map`, `excluded` (may be NULL) and `tax` must outlive the
   converter; the maps may grow between calls.  On a taxonomy that is no single tree a record whose taxa have no common
   ancestor is dropped and counted (the tool hangs or throws). */
typedef struct kaiju_gpu_converter kaiju_gpu_converter;
int kaiju_gpu_converter_create(const kaiju_gpu_taxonomy *tax, const uint64_t *include_ids, uint32_t n_include, const kaiju_gpu_accmap *map,
                               const kaiju_gpu_accmap *excluded, int add_acc, kaiju_gpu_converter **out);
/* The same with a rule set.  KAIJU_GPU_CONVERT_RULES_NR: kaiju_gpu_converter_create without an excluded map.
   KAIJU_GPU_CONVERT_RULES_REFSEQ: what kaiju-convertRefSeq.cpp:205-265 writes - the one accession of a header is [1, first
   space), a header without a space is dropped, '\x01' is a byte like any other, the record's taxon is the entry's (no LCA, no
   excluded set); the output is built as above.  `map` must have been made with the same rule set (KAIJU_GPU_ERR_ARG).  In
   kaiju_gpu_convert_info n_entries counts the headers that have a space, n_hits those found; dropped_excluded and
   dropped_no_lca stay 0. */
int kaiju_gpu_converter_create_rules(const kaiju_gpu_taxonomy *tax, const uint64_t *include_ids, uint32_t n_include, const kaiju_gpu_accmap *map,
                                     int rules, int add_acc, kaiju_gpu_converter **out);
void kaiju_gpu_converter_free(kaiju_gpu_converter *c);
typedef struct kaiju_gpu_convert_info {
  uint64_t text_bytes;             /* of the whole output, also when it overflowed                                         */
  uint64_t written_bytes;          /* of the whole records in front of out_cap                                             */
  uint64_t n_records, n_kept;
  uint64_t dropped_excluded;       /* an accession of the excluded set                                                     */
  uint64_t dropped_no_taxon;       /* no accession with a taxon > 0                                                        */
  uint64_t dropped_not_included;   /* no id of the include list above the taxon                                            */
  uint64_t dropped_no_lca;         /* the taxa have no common ancestor: the tree is no tree                                */
  uint64_t n_entries, n_hits;      /* entries of the headers / those the map holds with a taxon > 0                        */
  uint64_t n_lines;
  uint32_t overflow, reserved0;    /* 1: the text is longer than out_cap                                                   */
  uint64_t reserved[4];
} kaiju_gpu_convert_info;          /* 128 bytes */
/* All pointers device pointers, d_text and d_out 16-byte aligned, 16 readable bytes behind the text, bytes <= 2^32 - 17; every
   pass is queued on `stream` (NULL: a stream of the object), nothing synchronises.  A record is written whole or not at all
   and no byte at or behind out_cap is touched.  One call at a time per object. */
int kaiju_gpu_convert_text_device(kaiju_gpu_converter *c, const void *d_text, uint64_t bytes, void *d_out, uint64_t out_cap,
                                  kaiju_gpu_convert_info *d_info, void *stream);
/* The same from and into host memory; blocks */
int kaiju_gpu_convert_text(kaiju_gpu_converter *c, const char *text, uint64_t bytes, char *out, uint64_t out_cap, kaiju_gpu_convert_info *info);
/* With KAIJU_GPU_CONVERT_TIMES=1 at create: the milliseconds of the last call's passes - lines, kinds, entries, decide,
   lengths and offsets, write, finish */
enum { KAIJU_GPU_CONVERT_PASSES = 7 };
int kaiju_gpu_convert_pass_ms(kaiju_gpu_converter *c, float *ms, uint32_t n);

/* ---- kaiju-gbk2faa: GenBank flat files to the protein FASTA of the index builder ---------------------------------- */
/* What util/kaiju-gbk2faa.pl writes for a block of GenBank flat-file text (kaiju_amd/csrc/gbk.hip; the rules: kj_gbk.h): per
   /translation a header line '>' protein id '_' taxon '\n' and one line of filtered letters per line of the translation.  A
   file is converted in blocks cut behind a '\n'; the object keeps what the script carries from line to line - the taxon and the
   protein id seen last, whether a translation is open - in device memory between calls.  kaiju_gpu_gbk_reset starts a new file. */
typedef struct kaiju_gpu_gbk kaiju_gpu_gbk;
int kaiju_gpu_gbk_create(int device_id, kaiju_gpu_gbk **out);
void kaiju_gpu_gbk_free(kaiju_gpu_gbk *g);
int kaiju_gpu_gbk_reset(kaiju_gpu_gbk *g);
typedef struct kaiju_gpu_gbk_info {
  uint64_t text_bytes;             /* of the whole output, also when it overflowed                                         */
  uint64_t written_bytes;          /* of the whole output lines in front of out_cap                                        */
  uint64_t n_lines;
  uint64_t lines_kind[5];          /* taxon, protein id, whole translation, translation opens, every other line            */
  uint64_t n_records;              /* headers                                                                              */
  uint64_t letters_kept, letters_dropped;   /* bytes of the printed spans the filter kept / dropped                        */
  uint64_t no_taxon_line;          /* line (from 1, of this text) of the first /translation in front of which no taxon was */
                                   /* seen, 0: none.  The script ends there with an empty file: nothing is written and the */
                                   /* sizes, records and letters are 0                                                     */
  uint32_t overflow, reserved0;    /* 1: the text is longer than out_cap                                                   */
  uint64_t reserved[3];
} kaiju_gpu_gbk_info;              /* 128 bytes */
/* All pointers device pointers, d_text and d_out 16-byte aligned, 16 readable bytes behind the text, bytes <= 2^32 - 17; every
   pass is queued on `stream` (NULL: a stream of the object), nothing synchronises unless scratch has to grow.  An output line is
   written whole or not at all and no byte at or behind out_cap is touched.  A call that overflows or reports no_taxon_line
   leaves the carried state as it was: the caller repeats it with text_bytes of room.  One call at a time per object. */
int kaiju_gpu_gbk_text_device(kaiju_gpu_gbk *g, const void *d_text, uint64_t bytes, void *d_out, uint64_t out_cap, kaiju_gpu_gbk_info *d_info,
                              void *stream);
/* The same from and into host memory; blocks */
int kaiju_gpu_gbk_text(kaiju_gpu_gbk *g, const char *text, uint64_t bytes, char *out, uint64_t out_cap, kaiju_gpu_gbk_info *info);
/* With KAIJU_GPU_CONVERT_TIMES=1 at create: the milliseconds of the last call's passes - lines, kinds, scans, lengths and
   offsets, write, finish */
enum { KAIJU_GPU_GBK_PASSES = 6 };
int kaiju_gpu_gbk_pass_ms(kaiju_gpu_gbk *g, float *ms, uint32_t n);

/* ---- the rows of kaiju2table (host only, no GPU) -------------------------------------------------------------- */
enum { KAIJU_TABLE_EXPAND_VIRUSES = 1, KAIJU_TABLE_FILTER_UNCLASSIFIED = 2, KAIJU_TABLE_FULL_PATH = 4 };   /* -e, -u, -p */
typedef struct kaiju_table_options {
  const char *rank;                /* -r: phylum, class, order, family, genus or species                                   */
  const char *ranks_csv;           /* -l, NULL: none.  Not together with KAIJU_TABLE_FULL_PATH; it must hold `rank`         */
  float min_percent;               /* -m, in [0, 100]; not together with min_count                                         */
  int32_t min_count;               /* -c, >= 0                                                                             */
  uint32_t flags;                  /* KAIJU_TABLE_*                                                                        */
  uint32_t reserved;
} kaiju_table_options;
/* The rows that kaiju2table.cpp:238-360 prints for one input file - no header row - from the entries and totals of
   kaiju_gpu_tally_result (in any order; `names` of any mode), `label` in the file column.  Returns KAIJU_GPU_OK with the size
   of the whole text in *n_bytes and its first min(size, cap) bytes in buf, or KAIJU_GPU_ERR_ARG for options the tool refuses. */
int kaiju_table_rows(const kaiju_taxon_names *names, const kaiju_gpu_tally_entry *entries, uint64_t n_entries,
                     const kaiju_gpu_tally_info *totals, const kaiju_table_options *opt, const char *label, char *buf, uint64_t cap,
                     uint64_t *n_bytes);

/* ---- the lines of kaiju -v on the device: hits and matches in, text out ------------------------------------ */
/* What stage 4 of the command line programs does on the host for kaiju / kaiju-multi WITH -v, as HIP passes
   (kaiju_amd/csrc/format_verbose.hip; the rules: kj_format_verbose.h): the decision of the three-column lines, and for a
   classified read "C\t<name>\t<taxon>\t<best>\t<ids>\t<accs>\t<peptides>\n" - the ids of the hit in ascending order, the sorted
   set of the accessions (names of the matched database sequences up to their last '_'), the peptides as k_vb_pack packs them.
   The accession strings come from a table of the index that is uploaded on request: */
/* Host only, no GPU: per sequence name the length of its prefix up to, not including, the last '_' and the rank of that prefix
   among the sorted distinct prefixes of all nseq names (std::string order; equal prefixes share a rank; 0xffffffff and length
   0: the name has no '_'). */
int kaiju_accession_ranks(const char *const *names, uint32_t nseq, uint32_t *rank, uint32_t *prefix_len);
/* The accession table of the index to its device: the prefixes as one blob, per sequence offset (8 bytes), length and rank (4
   each).  Explicit - a run without -v never pays for it - and idempotent; concurrent callers are serialised.  An index
   loaded with KAIJU_GPU_IDS_SEQUENCE: KAIJU_GPU_ERR_UNSUPPORTED. */
int kaiju_gpu_index_upload_accessions(kaiju_gpu_index *ix);
/* bytes of the table in HBM, 0 before the upload */
uint64_t kaiju_gpu_index_accession_bytes(const kaiju_gpu_index *ix);
typedef struct kaiju_gpu_format_verbose_info {
  uint64_t text_bytes;             /* size of the whole text, whether or not it fitted                                      */
  uint32_t n_records, n_classified;/* records formatted (= n), 'C' lines among them                                         */
  uint32_t overflow;               /* 1: text_bytes > out_cap; the whole lines that fit are written, no byte at or behind   */
                                   /* out_cap is touched                                                                    */
  uint32_t n_inexact;              /* records whose compact info carries KAIJU_HIT_INEXACT                                  */
  uint32_t n_truncated;            /* classified records whose peptides were cut (text_len > text_cap)                      */
  uint32_t reserved;
} kaiju_gpu_format_verbose_info;   /* 32 bytes */
/* All pointers are device pointers on the context's GPU.  d_hits: n hit records; d_recs: the n compact records k_lca makes of
   them; d_off: 2n + 1; d_n_acc: n; d_acc_iseq: n x KAIJU_GPU_MAX_ACC; d_text_pos (n) / d_text_len (n): where the peptides of
   record r lie in d_pep and how many there are (more than text_cap: cut there, counted in n_truncated); d_names_text:
   names_bytes (below 2^32 - 32) bytes the spans d_names (n) point into.  d_out must be 16-byte aligned (KAIJU_GPU_ERR_ARG
   otherwise).  Asynchronous on `stream` (NULL: the context's own); nothing waits for the host.  Without an uploaded accession
   table: KAIJU_GPU_ERR_ARG.  The scratch lives in the context and grows when a call needs more: 24 bytes per record and a
   shadow of the output of out_cap bytes (so out_cap is a capacity to choose with care, not a safe huge number). */
int kaiju_gpu_format_verbose_device(kaiju_gpu_ctx *ctx, const kaiju_gpu_hit *d_hits, const kaiju_gpu_compact *d_recs,
                                    const uint64_t *d_off, uint32_t n, int paired, const uint32_t *d_n_acc,
                                    const uint32_t *d_acc_iseq, const uint64_t *d_text_pos, const uint32_t *d_text_len,
                                    const void *d_pep, uint32_t text_cap, const void *d_names_text, uint64_t names_bytes,
                                    const kaiju_gpu_name_span *d_names, void *d_out, uint64_t out_cap,
                                    kaiju_gpu_format_verbose_info *d_info, void *stream);
/* The same with host pointers: what kaiju_gpu_classify_batch_verbose_packed returns (hits, vout, text_pos, text, text_bytes),
   the compact records and the names.  vout[r].text_len above text_cap is cut at text_cap; a record is counted as truncated
   when that happens or when vout[r].truncated is set.  Everything goes up, *info and the bytes written come down; blocks.
   out[0 .. out_cap): only the bytes of the lines written change. */
int kaiju_gpu_format_verbose(kaiju_gpu_ctx *ctx, const kaiju_gpu_hit *hits, const kaiju_gpu_verbose *vout, const uint64_t *text_pos,
                             const char *text, uint64_t text_bytes, uint32_t text_cap, const kaiju_gpu_compact *recs,
                             const uint64_t *off, uint32_t n, int paired, const char *names_text, uint64_t names_bytes,
                             const kaiju_gpu_name_span *names, char *out, uint64_t out_cap, kaiju_gpu_format_verbose_info *info);
/* Reads in, the text of kaiju -v out: the verbose classification of kaiju_gpu_classify_batch_verbose_packed, k_vb_pack, the LCA
   on the device and the passes above on the context's stream.  The one synchronisation inside is the read-back of the text's
   size in front of the write pass (the library owns and sizes the output).  *text (text_bytes bytes) stays valid until the next
   verbose call on this context.  No hit record, accession array or peptide string crosses to the host. */
int kaiju_gpu_classify_batch_verbose_text(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const char *seqs, const uint64_t *off,
                                          uint32_t n_reads, int paired, const char *names_text, uint64_t names_bytes,
                                          const kaiju_gpu_name_span *names, const char **text, uint64_t *text_bytes,
                                          kaiju_gpu_format_verbose_info *info);

/* ---- the lines of kaijux / kaijup on the device: hits in, text out ------------------------------------------ */
/* What stage 4 of the command line programs does on the host for kaijux / kaijup, with and without -v, as HIP passes
   (kaiju_amd/csrc/format_seq.hip; the rules: kj_format_seq.h): the decision of the three-column lines on the record
   {lca = n_ids ? 1 : 0, best, info = n_ids}; for a classified read "C\t<name>\t<best>\t<ids>\t<peptides>\n" - the names of the
   matched database sequences in ascending order of their numbers, each followed by ',', and with -v the peptides as k_vb_pack
   packs them -; for any other "U\t<name>\t0\n" if the read is gated and "U\t<name>\n" if not.  Which reads are gated is an
   argument: */
enum { KAIJU_GPU_U_RULE_NUCLEOTIDE = 0,  /* kaijux (with -p too): read 1 shorter than 3 x min_fragment_length, of a pair both mates */
       KAIJU_GPU_U_RULE_PROTEIN = 1 };   /* kaijup: read 1 shorter than min_fragment_length, or without a run of amino-acid letters
                                            of that length that (Greedy) scores min_score on the BLOSUM62 diagonal                */
/* The names of all sequences of the index to its device: one blob, per sequence an offset (8 bytes) and a length (4).  Explicit
   - a run that does not ask never pays for it - and idempotent; concurrent callers are serialised.  For indexes of either id
   mode.  A name longer than 2^24 bytes: KAIJU_GPU_ERR_UNSUPPORTED. */
int kaiju_gpu_index_upload_seq_names(kaiju_gpu_index *ix);
/* bytes of the table in HBM (blob + 12 per sequence), 0 before the upload */
uint64_t kaiju_gpu_index_seq_name_bytes(const kaiju_gpu_index *ix);
/* All pointers are device pointers on the context's GPU.  d_hits: n hit records of a context whose index was loaded with
   KAIJU_GPU_IDS_SEQUENCE (any other: KAIJU_GPU_ERR_ARG); d_off: 2n + 1; d_seqs: the reads d_off points into, looked at under
   KAIJU_GPU_U_RULE_PROTEIN only (NULL otherwise); d_pep == NULL: no peptide column (without -v), d_text_pos / d_text_len /
   text_cap are not looked at; else as in kaiju_gpu_format_verbose_device.  d_names_text / names_bytes / d_names / d_out /
   out_cap / d_info / stream and the scratch (24 bytes per record and a shadow of out_cap bytes) as there: d_out 16-byte
   aligned (KAIJU_GPU_ERR_ARG otherwise), asynchronous, nothing waits for the host.  Without an uploaded name table:
   KAIJU_GPU_ERR_ARG. */
int kaiju_gpu_format_seq_device(kaiju_gpu_ctx *ctx, const kaiju_gpu_hit *d_hits, const uint64_t *d_off, uint32_t n, int paired,
                                int u_rule, const void *d_seqs, const uint64_t *d_text_pos, const uint32_t *d_text_len,
                                const void *d_pep, uint32_t text_cap, const void *d_names_text, uint64_t names_bytes,
                                const kaiju_gpu_name_span *d_names, void *d_out, uint64_t out_cap,
                                kaiju_gpu_format_verbose_info *d_info, void *stream);
/* The same with host pointers.  seqs: off[2n] bytes (NULL unless KAIJU_GPU_U_RULE_PROTEIN).  text == NULL: no peptide column,
   vout and text_pos are not looked at; else vout[r].text_len letters at text + text_pos[r], cut at text_cap; a classified record
   is counted as truncated when that happens or when vout[r].truncated is set.  Everything goes up, *info and the bytes written
   come down; blocks.  out[0 .. out_cap): only the bytes of the lines written change. */
int kaiju_gpu_format_seq(kaiju_gpu_ctx *ctx, const kaiju_gpu_hit *hits, const uint64_t *off, uint32_t n, int paired, int u_rule,
                         const char *seqs, const kaiju_gpu_verbose *vout, const uint64_t *text_pos, const char *text,
                         uint64_t text_bytes, uint32_t text_cap, const char *names_text, uint64_t names_bytes,
                         const kaiju_gpu_name_span *names, char *out, uint64_t out_cap, kaiju_gpu_format_verbose_info *info);
/* Reads in, the text of kaijux / kaijup out, on the context's stream: without `verbose` the plain classification of
   kaiju_gpu_classify_batch, with it the verbose classification and k_vb_pack as kaiju_gpu_classify_batch_verbose_text queues
   them, then the passes above.  The one synchronisation inside is the read-back of the text's size in front of the write pass
   (the library owns and sizes the output).  *text (text_bytes bytes) stays valid until the next verbose or text call on this
   context.  No hit record, sequence number or peptide string crosses to the host.  A context whose index was not loaded with
   KAIJU_GPU_IDS_SEQUENCE: KAIJU_GPU_ERR_ARG. */
int kaiju_gpu_classify_batch_seq_text(kaiju_gpu_ctx *ctx, const char *seqs, const uint64_t *off, uint32_t n_reads, int paired,
                                      int verbose, int u_rule, const char *names_text, uint64_t names_bytes,
                                      const kaiju_gpu_name_span *names, const char **text, uint64_t *text_bytes,
                                      kaiju_gpu_format_verbose_info *info);

/* ---- several processes of a node, one per GPU: the gather --------------- */
/* BASELINE north star: "reads shard embarrassingly across the GPUs of one node with the index replicated per GPU and per-GPU
   hit lists gathered with a single RCCL gather over xGMI".  The reference has no exchange (its threads append to one output
   stream under a mutex, ConsumerThread.cpp:847-856; the thread fan-out is kaiju.cpp:250-257); here every rank classifies its
   shard, the device LCA turns the hits into 16-byte records and ONE collective per batch brings them to the rank that
   writes the output.  kaiju_gpu_comm_create: rank 0 makes the communicator's id and hands it over through `rendezvous_path`
   (any path all ranks of the job see and may write next to, e.g. under /dev/shm; up to two minutes for everybody to arrive).
   The path need not be fresh: rank r > 0 announces itself with a random nonce in `<path>.r<r>`, takes the id only from a file
   that carries that nonce and removes its nonce file; rank 0 removes whatever lay at `<path>` before, and the file itself once
   every rank has acknowledged - a file left by an earlier job is never taken for this job's id.  Two jobs must not use ONE
   path at the same time.  librccl is opened on the first call (dlopen): nothing links it, a single-GPU run never loads it.
   kaiju_gpu_gather_compact: n records of EVERY rank (the same n everywhere) into d_recv on `root`, rank r's at d_recv + r * n;
   d_recv is ignored elsewhere.  Asynchronous on `stream` (a hipStream_t; kaiju_gpu_get_stream() of the context that wrote
   d_send orders it behind the batch).  Without a HIP device: KAIJU_GPU_ERR_NO_DEVICE. */
typedef struct kaiju_gpu_comm kaiju_gpu_comm;
int kaiju_gpu_comm_create(const char *rendezvous_path, int rank, int world, int device_id, kaiju_gpu_comm **out);
void kaiju_gpu_comm_destroy(kaiju_gpu_comm *comm);
int kaiju_gpu_comm_rank(const kaiju_gpu_comm *comm);
int kaiju_gpu_comm_world(const kaiju_gpu_comm *comm);
int kaiju_gpu_gather_compact(kaiju_gpu_comm *comm, const kaiju_gpu_compact *d_send, uint32_t n, kaiju_gpu_compact *d_recv,
                             int root, void *stream);
const char *kaiju_gpu_comm_last_error(void);
/* the librccl the gather runs on ("" before the first communicator): the one that lies next to the HIP runtime this process
   uses - a Python host may hold two ROCm stacks, the system's and the one bundled with torch */
const char *kaiju_gpu_comm_library(void);

int kaiju_finalize_hits(kaiju_taxonomy *t, const kaiju_gpu_params *p, double db_length,
                        const kaiju_gpu_hit *hits, const uint64_t *off, uint32_t n_reads,
                        int paired, kaiju_result *out);

#ifdef __cplusplus
}
#endif
#endif /* KAIJU_GPU_H */
