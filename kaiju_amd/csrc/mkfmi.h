/* mkfmi.h - index construction, TEST / BENCHMARK INFRASTRUCTURE (not part of the product boundary include/kaiju_gpu.h).
 *
 * Building a .fmi is the reference's off-line step (kaiju-mkbwt + kaiju-mkfmi) and out of scope of the classification path
 * (OUT OF SCOPE).  There is no network on the GPU box and the reference's binaries do not travel there, so
 * bench.py and the tests need a way to make the indexes they classify on: this builder writes byte-identical files
 * (tests/test_mkfmi_pin.py).  It is compiled into a library of its own, kaiju_amd/libkaiju_mkfmi.so (host only, no HIP);
 * libkaiju_gpu.so does not contain it.
 *
 * A third library, kaiju_amd/libkaiju_mkfmi_gpu.so, is the same builder compiled with -DKAIJU_MKFMI_GPU plus sufsort.hip and
 * fmibuild.hip: it has every entry point of the host library and the *_device ones below, which sort the suffixes on a GPU
 * (kj_sufsort.h) and by default leave everything else - BWT, sequence ranks, SA samples, byte coding, checkpoints, the file -
 * to the same host code, so the file is byte for byte the host builder's (tests/test_gpu_sufsort.py).  Asked to
 * (kaiju_build_fmi_device_ex with KAIJU_FMI_STAGES_DEVICE) they also run the stages behind the sort on the GPU (kj_fmibuild.h):
 * text, ranks and suffix array stay in device memory, five passes make the arrays of the file there, the host downloads what it
 * writes and writes it with the one copy of the header / names / write code - the same bytes again (tests/test_gpu_fmibuild.py).
 * The host library does not have the *_device entry points and needs no HIP runtime.
 */
#ifndef KAIJU_MKFMI_H
#define KAIJU_MKFMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes: the values of include/kaiju_gpu.h's enum (0 ok, -1 bad argument, -2 file error; the device entry points also
   -4 no HIP device, -5 a HIP call failed, -6 not enough free device memory) */
#ifndef KAIJU_GPU_H
enum { KAIJU_GPU_OK = 0, KAIJU_GPU_ERR_ARG = -1, KAIJU_GPU_ERR_IO = -2, KAIJU_GPU_ERR_NO_DEVICE = -4, KAIJU_GPU_ERR_HIP = -5, KAIJU_GPU_ERR_NOMEM = -6 };
#endif

/* Protein FASTA -> .fmi, format-compatible with the reference's kaiju-mkbwt (-a
   ACDEFGHIKLMNPQRSTVWY -e chpt_exp, util/kaiju-makedb:373) followed by kaiju-mkfmi
   (bwt/mkbwt.c:922-1099, bwt/mkfmi.c:21-97); the reference binary reads the result.
   threads <= 0: all hardware threads.  Host only. */
int kaiju_build_fmi(const char *faa_path, const char *out_fmi_path, int threads, int chpt_exp);
/* The .fmi of the database in which every sequence of the FASTA occurs `copies` times in a row, without sorting it again (equal
   suffixes order by file position, so every row of the file's own index becomes `copies` rows); byte for byte what
   kaiju_build_fmi writes for the FASTA with the repeats spelled out.  Test / benchmark infrastructure: an index of 2^32 rows
   and more (the layout with 64-bit positions) from a small FASTA in seconds.  copy_taxids (may be NULL): copy t of sequence
   number i, named X_<id>, is named X_<copy_taxids[(i + t) % n_copy_taxids]>. */
int kaiju_build_fmi_replicated(const char *faa_path, const char *out_fmi_path, int threads, int chpt_exp, uint64_t copies,
                               const uint64_t *copy_taxids, uint32_t n_copy_taxids);
const char *kaiju_build_fmi_error(void);

/* ---- libkaiju_mkfmi_gpu.so only: the suffix sort on the device ------------------------------------------------------------ */
enum { KAIJU_SUFSORT_STATS_ROUNDS = 16 };
typedef struct kaiju_sufsort_stats {
  uint32_t rounds;                                 /* round 1 (keys of 12 symbols) and the doubling rounds; 0 without a suffix */
  uint32_t reserved;
  uint64_t active[KAIJU_SUFSORT_STATS_ROUNDS];     /* suffixes not yet final in front of round 1, 2, ...: active[0] = all */
  float ms_sort;                                   /* HIP events around upload, sort and download */
  float reserved2;
} kaiju_sufsort_stats;
/* kaiju_build_fmi / kaiju_build_fmi_replicated with the suffixes sorted on device `device_id`; the same bytes.  A file below
   0xf0000000 bytes is sorted with 32-bit positions, a bigger one with 64-bit positions (the wide instantiation of the same
   sort, kj_sufsort.h; ranks below 2^40).  Under KAIJU_MKFMI_FORCE64 on a small file the device sorts in 32 bits and the builder
   widens the result, with KAIJU_MKFMI_DEVICE_WIDE=1 as well it runs the wide sort (a test switch).  A device_id that does not
   exist: KAIJU_GPU_ERR_ARG.  The sort's scratch - about 33 bytes per symbol narrow (ss_scratch_bytes), 49 bytes per symbol wide
   (ss_scratch_bytes_wide: text 1, ranks 8, keys 2 x 8, positions 2 x 8, active list 8), plus rocPRIM's temporary storage - is
   compared with the free device memory before anything is allocated: KAIJU_GPU_ERR_NOMEM with both numbers. */
int kaiju_build_fmi_device(const char *faa_path, const char *out_fmi_path, int threads, int chpt_exp, int device_id);
int kaiju_build_fmi_replicated_device(const char *faa_path, const char *out_fmi_path, int threads, int chpt_exp, uint64_t copies,
                                      const uint64_t *copy_taxids, uint32_t n_copy_taxids, int device_id);
/* The sorter alone.  Host pointers, blocking: text up, positions down.  text[0, tlen): codes 0 .. 20, the last one 0;
   sa_out: room for tlen minus the number of terminators; *n_out: how many were written.  tlen >= 0xf0000000 is refused
   (KAIJU_GPU_ERR_ARG) before the text is looked at: sa_out has 32-bit positions.  stats may be NULL. */
int kaiju_suffix_sort_device(const uint8_t *text, uint64_t tlen, int device_id, uint32_t *sa_out, uint64_t *n_out, kaiju_sufsort_stats *stats);
/* The same with 64-bit positions: always the wide instantiation, whatever the length.  tlen + rank_bias >= 2^40 is refused
   (KAIJU_GPU_ERR_ARG) before the text is looked at.  rank_bias is a test hook and 0 otherwise: every rank inside the sort is
   rank_bias higher, so that a small text carries ranks and round keys beyond 2^32 through the kernels; the result does not
   depend on it. */
int kaiju_suffix_sort_device_wide(const uint8_t *text, uint64_t tlen, int device_id, uint64_t *sa_out, uint64_t *n_out, kaiju_sufsort_stats *stats,
                                  uint64_t rank_bias);


/* ---- the arrays of a .fmi from a text, without a file (both libraries) ------------------------------------------------------
   text[0, tlen): letter codes 1 .. 20 and a terminator 0 behind every sequence, the last symbol a terminator; `copies` and
   chpt_exp as above.  kaiju_fmi_arrays_sizes fills the sizes of *a (everything above the pointers); the caller then points the
   pointers at buffers of those sizes and calls kaiju_fmi_arrays_host, which sorts on the host and runs the host stages.
   recode = 0 leaves the BWT letters raw (startLcode is computed all the same). */
typedef struct kaiju_fmi_arrays {
  uint64_t nseq, bwtlen;                           /* sequences of the text (not times copies); rows of the output = tlen * copies */
  uint64_t n_samples_bytes, n_index1, n_index2;    /* ncheck * nbytes bytes; N1 * 21 int64; N2 * 21 uint16 */
  int64_t ncheck;
  int32_t nbytes, sbits, pbits, N1, N2, reserved;
  uint32_t *read_of_rank;                          /* [nseq]: the file index of the sequence with sorted rank r */
  uint8_t *samples;                                /* [n_samples_bytes], big-endian entries of nbytes */
  uint8_t *bwt;                                    /* [bwtlen] */
  int64_t *index1;                                 /* [n_index1] */
  uint16_t *index2;                                /* [n_index2] */
  int32_t startLcode[22];
} kaiju_fmi_arrays;
int kaiju_fmi_arrays_sizes(const uint8_t *text, uint64_t tlen, uint64_t copies, int chpt_exp, kaiju_fmi_arrays *a);
int kaiju_fmi_arrays_host(const uint8_t *text, uint64_t tlen, uint64_t copies, int chpt_exp, int threads, int recode, kaiju_fmi_arrays *a);

/* ---- libkaiju_mkfmi_gpu.so only: the stages behind the sort on the device (kj_fmibuild.h, fmibuild.hip) ------------------------ */
enum { KAIJU_FMI_STAGES_HOST = 0, KAIJU_FMI_STAGES_DEVICE = 1 };
enum { KAIJU_FMI_STAGE_BWT = 1, KAIJU_FMI_STAGE_RANKS = 2, KAIJU_FMI_STAGE_SAMPLES = 4, KAIJU_FMI_STAGE_CHECKPOINTS = 8, KAIJU_FMI_STAGE_RECODE = 16 };
typedef struct kaiju_fmi_build_stats {
  uint32_t device_stages;                          /* KAIJU_FMI_STAGE_* of the stages that ran on the device; 0 with the host stages */
  uint32_t reserved;
  float ms_bwt, ms_ranks, ms_samples, ms_checkpoints, ms_recode;   /* HIP events around each pass (ms_samples: replication + samples) */
  float ms_download;                               /* ... and around the download of read_of_rank, samples, index2 and BWT */
  uint64_t device_bytes;                           /* what the size check compared with the free device memory */
  kaiju_sufsort_stats sort;                        /* (ms_sort without a download: SA stays on the device) */
} kaiju_fmi_build_stats;
/* kaiju_build_fmi_replicated_device with a choice of where the stages behind the sort run.  KAIJU_FMI_STAGES_HOST: what
   kaiju_build_fmi_replicated_device does.  KAIJU_FMI_STAGES_DEVICE: on the device; the same bytes.  Any other value:
   KAIJU_GPU_ERR_ARG.  The device memory needed - the sort's scratch that is kept plus tlen * copies bytes of BWT, samples,
   index2 and piece counts (kj_fmibuild.h: fb_scratch_bytes) - is compared with the free device memory before anything is
   allocated: KAIJU_GPU_ERR_NOMEM with both numbers, and no output file.  The device stages have 32-bit positions: where the wide
   sort would be chosen (a file of 0xf0000000 bytes and more, or KAIJU_MKFMI_DEVICE_WIDE set) KAIJU_FMI_STAGES_DEVICE is
   KAIJU_GPU_ERR_ARG, without an output file; stages = host builds such a file.  stats may be NULL. */
int kaiju_build_fmi_device_ex(const char *faa_path, const char *out_fmi_path, int threads, int chpt_exp, uint64_t copies,
                              const uint64_t *copy_taxids, uint32_t n_copy_taxids, int device_id, int stages, kaiju_fmi_build_stats *stats);
/* kaiju_fmi_arrays_host with the sort and all five stages on device `device_id`: the analogue of kaiju_suffix_sort_device.
   Host pointers, blocking.  32-bit positions: tlen >= 0xf0000000 is KAIJU_GPU_ERR_ARG.  stats may be NULL. */
int kaiju_fmi_arrays_device(const uint8_t *text, uint64_t tlen, uint64_t copies, int chpt_exp, int device_id, int recode, kaiju_fmi_arrays *a,
                            kaiju_fmi_build_stats *stats);

#ifdef __cplusplus
}
#endif

#endif
