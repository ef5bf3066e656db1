// capi_text.hip - the text half of the C-ABI (include/kaiju_gpu.h): the host entry points of record ingest (ingest.hip) and of
// the four formatters (format.hip, format_names.hip, format_verbose.hip, format_seq.hip).  No kernel is defined here: the
// passes are launched by kj_*_launch / kj_*_lengths / kj_*_write of those files, the classification by capi.hip.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "capi_internal.h"
#include "kj_ingest.h"
#include "kj_format.h"
#include "kj_format_verbose.h"
#include "kj_format_seq.h"
#include "kj_format_names.h"
// Libraries linked from a source list of their own need not hold ingest.hip, format.hip, format_verbose.hip with accessions.cpp,
// format_seq.hip or format_names.hip: their functions are weak references here, and without them the entry points below say
// KAIJU_GPU_ERR_UNSUPPORTED.  kaiju_amd/build.py always links them all.
__attribute__((weak)) decltype(kj_ingest_launch) kj_ingest_launch;
__attribute__((weak)) decltype(kj_format_launch) kj_format_launch;
__attribute__((weak)) decltype(kj_fv_lengths) kj_fv_lengths;
__attribute__((weak)) decltype(kj_fv_write) kj_fv_write;
extern "C" __attribute__((weak)) decltype(kaiju_accession_ranks) kaiju_accession_ranks;
__attribute__((weak)) decltype(kj_fs_lengths) kj_fs_lengths;
__attribute__((weak)) decltype(kj_fs_write) kj_fs_write;
__attribute__((weak)) decltype(kj_fn_launch) kj_fn_launch;
__attribute__((weak)) decltype(kj_fn_device) kj_fn_device;
extern "C" __attribute__((weak)) decltype(kaiju_gpu_taxon_names_max_annotation) kaiju_gpu_taxon_names_max_annotation;

using namespace kj;

// ---- record extraction on the device (ingest.hip) ---------------------------------------------------------------
static int no_ingest() { return kj_ingest_launch ? KAIJU_GPU_OK : fail(KAIJU_GPU_ERR_UNSUPPORTED, "this library was linked without ingest.hip"); }

extern "C" int kaiju_gpu_parse_block_device(kaiju_gpu_ctx *ctx, const void *d_text1, uint64_t bytes1, const void *d_text2, uint64_t bytes2,
                                            int fastq, int keep_names, uint32_t rec_cap, void *d_seqs, uint64_t *d_off,
                                            kaiju_gpu_name_span *d_names, kaiju_gpu_parse_info *d_info, void *stream) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_ingest()) return rc;
  if (!ctx) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  KJ_HIP(hipSetDevice(ctx->ix->device));
  const char *err = "";
  const int rc = kj_ingest_launch(ctx->ingest, stream ? static_cast<hipStream_t>(stream) : ctx->stream, d_text1, bytes1, d_text2, bytes2,
                                  fastq, keep_names, rec_cap, d_seqs, d_off, d_names, d_info, &err);
  return rc ? fail(rc, err) : KAIJU_GPU_OK;
  });
}

// text up, the passes queued on the context's stream, *info back (blocks until it is there); the other results stay in
// ctx->h_seqs / h_off / ing_names
static int parse_host_text(kaiju_gpu_ctx *ctx, const char *text1, uint64_t bytes1, const char *text2, uint64_t bytes2, int fastq,
                           int keep_names, uint32_t rec_cap, kaiju_gpu_parse_info *info) {
  if (!ctx || !info || (!text1 && bytes1) || (!text2 && bytes2)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (bytes1 > kji::kMaxBytes || bytes2 > kji::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 bytes");
  if (int rc0 = no_ingest()) return rc0;
  KJ_HIP(hipSetDevice(ctx->ix->device));
  int rc;
  if ((rc = ensure(ctx->ing_text1, bytes1 + 64))) return rc;
  if (text2 && (rc = ensure(ctx->ing_text2, bytes2 + 64))) return rc;
  if ((rc = ensure(ctx->h_seqs, bytes1 + bytes2 + 64))) return rc;
  if ((rc = ensure(ctx->h_off, (2 * (size_t)rec_cap + 1) * 8))) return rc;
  if ((rc = ensure(ctx->ing_names, ((size_t)rec_cap + 1) * sizeof(kaiju_gpu_name_span)))) return rc;
  if ((rc = ensure(ctx->ing_info, sizeof(kaiju_gpu_parse_info)))) return rc;
  hipStream_t s = ctx->stream;
  if (bytes1) KJ_HIP(hipMemcpyAsync(ctx->ing_text1.p, text1, bytes1, hipMemcpyHostToDevice, s));
  if (bytes2) KJ_HIP(hipMemcpyAsync(ctx->ing_text2.p, text2, bytes2, hipMemcpyHostToDevice, s));
  const char *err = "";
  rc = kj_ingest_launch(ctx->ingest, s, ctx->ing_text1.p, bytes1, text2 ? ctx->ing_text2.p : nullptr, bytes2, fastq, keep_names, rec_cap,
                        ctx->h_seqs.p, static_cast<uint64_t *>(ctx->h_off.p), static_cast<kaiju_gpu_name_span *>(ctx->ing_names.p),
                        static_cast<kaiju_gpu_parse_info *>(ctx->ing_info.p), &err);
  if (rc) return fail(rc, err);
  KJ_HIP(hipMemcpyAsync(info, ctx->ing_info.p, sizeof *info, hipMemcpyDeviceToHost, s));
  KJ_HIP(hipStreamSynchronize(s));
  return KAIJU_GPU_OK;
}
static uint32_t reads_emitted(const kaiju_gpu_parse_info &info, bool paired, uint32_t rec_cap) {
  return std::min(rec_cap, paired ? std::min(info.n_records, info.n_records2) : info.n_records);
}

extern "C" int kaiju_gpu_parse_block(kaiju_gpu_ctx *ctx, const char *text1, uint64_t bytes1, const char *text2, uint64_t bytes2, int fastq,
                                     int keep_names, uint32_t rec_cap, char *seqs, uint64_t *off, kaiju_gpu_name_span *names,
                                     kaiju_gpu_parse_info *info) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (!off || (!names && rec_cap) || (!seqs && bytes1 + bytes2)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (int rc = parse_host_text(ctx, text1, bytes1, text2, bytes2, fastq, keep_names, rec_cap, info)) return rc;
  const uint32_t n = reads_emitted(*info, text2 != nullptr, rec_cap);
  hipStream_t s = ctx->stream;
  if (info->seq_bytes) KJ_HIP(hipMemcpyAsync(seqs, ctx->h_seqs.p, info->seq_bytes, hipMemcpyDeviceToHost, s));
  KJ_HIP(hipMemcpyAsync(off, ctx->h_off.p, (2 * (size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
  if (n) KJ_HIP(hipMemcpyAsync(names, ctx->ing_names.p, (size_t)n * sizeof(kaiju_gpu_name_span), hipMemcpyDeviceToHost, s));
  KJ_HIP(hipStreamSynchronize(s));
  return KAIJU_GPU_OK;
  });
}

// text in, the records parsed and classified on the device (blocks for the parse's counts only): *n records of paired or
// single reads, their 16-byte records in ctx->h_compact, offsets in h_off, name spans in ing_names, text 1 in ing_text1
static int classify_text_device(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const char *text1, uint64_t bytes1, const char *text2,
                                uint64_t bytes2, int fastq, int keep_names, uint32_t rec_cap, kaiju_gpu_parse_info *info, uint32_t *n, bool *paired) {
  if (int rc = parse_host_text(ctx, text1, bytes1, text2, bytes2, fastq, keep_names, rec_cap, info)) return rc;
  if (info->overflow) return fail(KAIJU_GPU_ERR_ARG, "the text holds more records than rec_cap");
  *paired = text2 != nullptr;
  *n = reads_emitted(*info, *paired, rec_cap);
  int rc;
  if ((rc = ensure(ctx->h_compact, ((size_t)*n + 1) * sizeof(kaiju_gpu_compact)))) return rc;
  if (*n == 0) return KAIJU_GPU_OK;
  if ((rc = kaiju_gpu_set_max_read_length(ctx, std::max(1u, info->max_mate_len)))) return rc;
  if ((rc = ensure(ctx->h_hits, (size_t)*n * sizeof(kaiju_gpu_hit)))) return rc;
  return kaiju_gpu_classify_batch_device_compact(ctx, t, ctx->h_seqs.p, info->seq_bytes, static_cast<const uint64_t *>(ctx->h_off.p), *n, *paired ? 1 : 0,
                                                 static_cast<kaiju_gpu_hit *>(ctx->h_hits.p), static_cast<kaiju_gpu_compact *>(ctx->h_compact.p), ctx->stream);
}

extern "C" int kaiju_gpu_classify_text_compact(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const char *text1, uint64_t bytes1,
                                               const char *text2, uint64_t bytes2, int fastq, int keep_names, uint32_t rec_cap,
                                               kaiju_gpu_compact *out, uint64_t *off, kaiju_gpu_name_span *names,
                                               kaiju_gpu_parse_info *info) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (!ctx || !t || !off || (!names && rec_cap) || (!out && rec_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (t->device != ctx->ix->device) return fail(KAIJU_GPU_ERR_ARG, "taxonomy lives on another device");
  uint32_t n;
  bool paired;
  if (int rc = classify_text_device(ctx, t, text1, bytes1, text2, bytes2, fastq, keep_names, rec_cap, info, &n, &paired)) return rc;
  hipStream_t s = ctx->stream;
  KJ_HIP(hipMemcpyAsync(off, ctx->h_off.p, (2 * (size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
  if (n) {
    KJ_HIP(hipMemcpyAsync(names, ctx->ing_names.p, (size_t)n * sizeof(kaiju_gpu_name_span), hipMemcpyDeviceToHost, s));
    KJ_HIP(hipMemcpyAsync(out, ctx->h_compact.p, (size_t)n * sizeof(kaiju_gpu_compact), hipMemcpyDeviceToHost, s));
  }
  KJ_HIP(hipStreamSynchronize(s));
  return KAIJU_GPU_OK;
  });
}

// ---- the output lines on the device (format.hip) ------------------------------------------------------------------
static int no_format() { return kj_format_launch ? KAIJU_GPU_OK : fail(KAIJU_GPU_ERR_UNSUPPORTED, "this library was linked without format.hip"); }
extern "C" uint64_t kaiju_gpu_format_bound(uint64_t bytes1, uint32_t n) { return bytes1 + (uint64_t)kjf::kLineExtra * n; }
// what every formatter takes from the context: the checks they share (behind the caller's own of the index's id_mode, whose
// wording differs), and the parameters of the decision
static int format_params(const kaiju_gpu_ctx *ctx, int paired, kjf::Params &P) {
  if (paired && ctx->params.input_is_protein) return fail(KAIJU_GPU_ERR_ARG, "protein reads have no mates");
  if (!ctx->fmt_pw_ok) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "a score beyond the table of the E-value gate has a factor other than +0.0");
  P.db_length = ctx->ix->info.db_length;
  P.min_evalue = ctx->params.min_evalue;
  P.gate = ctx->params.mode == 1 && ctx->params.use_evalue ? 1 : 0;
  P.protein = ctx->params.input_is_protein ? 1 : 0;
  P.paired = paired ? 1 : 0;
  return KAIJU_GPU_OK;
}
template <class Info>
constexpr bool kWithNames = std::is_same<Info, kaiju_gpu_format_names_info>::value;
// the passes of the three-column lines on stream s, all pointers device pointers; Info = kaiju_gpu_format_names_info: with the
// taxon names of `names` (format_names.hip), else names and drop are not looked at (format.hip)
template <class Info>
static int format_launch(kaiju_gpu_ctx *ctx, hipStream_t s, const kaiju_gpu_compact *d_recs, const uint64_t *d_off, uint32_t n, int paired,
                         const void *d_text1, uint64_t bytes1, const kaiju_gpu_name_span *d_names, const kaiju_gpu_taxon_names *names, int drop,
                         void *d_out, uint64_t out_cap, Info *d_info) {
  if constexpr (kWithNames<Info>) {
    if (!names) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
    if (kj_fn_device(names) != ctx->ix->device) return fail(KAIJU_GPU_ERR_ARG, "the taxon names live on another device");
  }
  if (ctx->ix->id_mode != KAIJU_GPU_IDS_TAXON)
    return fail(KAIJU_GPU_ERR_UNSUPPORTED, kWithNames<Info> ? "the lines of kaijux / kaijup carry no taxon" : "the lines of kaijux / kaijup are not made on the device");
  kjf::Params P{};
  if (int rc = format_params(ctx, paired, P)) return rc;
  const char *err = "";
  const double *pw = static_cast<const double *>(ctx->fmt_pw.p);
  int rc;
  if constexpr (kWithNames<Info>) rc = kj_fn_launch(ctx->format_n, s, P, pw, d_recs, d_off, n, d_text1, bytes1, d_names, names, drop, d_out, out_cap, d_info, &err);
  else rc = kj_format_launch(ctx->format, s, P, pw, d_recs, d_off, n, d_text1, bytes1, d_names, d_out, out_cap, d_info, &err);
  return rc ? fail(rc, err) : KAIJU_GPU_OK;
}

extern "C" int kaiju_gpu_format_compact_device(kaiju_gpu_ctx *ctx, const kaiju_gpu_compact *d_recs, const uint64_t *d_off, uint32_t n, int paired,
                                               const void *d_text1, uint64_t bytes1, const kaiju_gpu_name_span *d_names, void *d_out,
                                               uint64_t out_cap, kaiju_gpu_format_info *d_info, void *stream) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format()) return rc;
  if (!ctx) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  KJ_HIP(hipSetDevice(ctx->ix->device));
  return format_launch(ctx, stream ? static_cast<hipStream_t>(stream) : ctx->stream, d_recs, d_off, n, paired, d_text1, bytes1, d_names, nullptr, 0,
                       d_out, out_cap, d_info);
  });
}

// *info (one of the three kaiju_gpu_format_*_info) from d_info and the bytes the passes of st wrote from d_out to the host; blocks
template <class Info>
static int format_download(hipStream_t s, const kjl::Lines &st, const DevBuf &d_info, const DevBuf &d_out, char *out, uint64_t out_cap, Info *info) {
  KJ_HIP(hipMemcpyAsync(info, d_info.p, sizeof *info, hipMemcpyDeviceToHost, s));
  KJ_HIP(hipStreamSynchronize(s));
  uint64_t written = info->text_bytes;
  if (info->overflow) KJ_HIP(hipMemcpy(&written, st.written, sizeof written, hipMemcpyDeviceToHost));
  if (written > out_cap) return fail(KAIJU_GPU_ERR_HIP, "the format passes report more bytes than the capacity");
  if (written) KJ_HIP(hipMemcpy(out, d_out.p, written, hipMemcpyDeviceToHost));
  return KAIJU_GPU_OK;
}

// the inputs of the three-column lines (with or without names) from the host to ctx->ing_text1 / h_compact / h_off /
// ing_names, and room for the output in fmt_out / fmt_info
static int format_stage(kaiju_gpu_ctx *ctx, const kaiju_gpu_compact *recs, const uint64_t *off, uint32_t n, const char *text1, uint64_t bytes1,
                        const kaiju_gpu_name_span *names, uint64_t out_cap, size_t info_bytes) {
  int rc;
  if ((rc = ensure(ctx->ing_text1, bytes1 + 64))) return rc;
  if ((rc = ensure(ctx->h_compact, ((size_t)n + 1) * sizeof(kaiju_gpu_compact)))) return rc;
  if ((rc = ensure(ctx->h_off, (2 * (size_t)n + 1) * 8))) return rc;
  if ((rc = ensure(ctx->ing_names, ((size_t)n + 1) * sizeof(kaiju_gpu_name_span)))) return rc;
  if ((rc = ensure(ctx->fmt_out, out_cap + 64))) return rc;
  if ((rc = ensure(ctx->fmt_info, info_bytes))) return rc;
  hipStream_t s = ctx->stream;
  if (bytes1) KJ_HIP(hipMemcpyAsync(ctx->ing_text1.p, text1, bytes1, hipMemcpyHostToDevice, s));
  if (n) {
    KJ_HIP(hipMemcpyAsync(ctx->h_compact.p, recs, (size_t)n * sizeof(kaiju_gpu_compact), hipMemcpyHostToDevice, s));
    KJ_HIP(hipMemcpyAsync(ctx->h_off.p, off, (2 * (size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    KJ_HIP(hipMemcpyAsync(ctx->ing_names.p, names, (size_t)n * sizeof(kaiju_gpu_name_span), hipMemcpyHostToDevice, s));
  }
  return KAIJU_GPU_OK;
}
// format_launch on what format_stage / classify_text_device left in the context, then the download
template <class Info>
static int format_staged(kaiju_gpu_ctx *ctx, uint32_t n, int paired, uint64_t bytes1, const kaiju_gpu_taxon_names *names, int drop, char *out,
                         uint64_t out_cap, Info *info) {
  const int rc = format_launch(ctx, ctx->stream, static_cast<const kaiju_gpu_compact *>(ctx->h_compact.p), static_cast<const uint64_t *>(ctx->h_off.p),
                               n, paired, ctx->ing_text1.p, bytes1, static_cast<const kaiju_gpu_name_span *>(ctx->ing_names.p), names, drop,
                               ctx->fmt_out.p, out_cap, static_cast<Info *>(ctx->fmt_info.p));
  return rc ? rc : format_download(ctx->stream, kWithNames<Info> ? ctx->format_n : ctx->format, ctx->fmt_info, ctx->fmt_out, out, out_cap, info);
}
// what kaiju_gpu_classify_text_to_text and .._names do behind their own guards and NULL checks
template <class Info>
static int text_to_text(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const char *text1, uint64_t bytes1, const char *text2, uint64_t bytes2,
                        int fastq, int keep_names, uint32_t rec_cap, const kaiju_gpu_taxon_names *names, int drop, char *out_text,
                        uint64_t out_cap, kaiju_gpu_parse_info *info_parse, Info *info_format) {
  if (t->device != ctx->ix->device) return fail(KAIJU_GPU_ERR_ARG, "taxonomy lives on another device");
  if (bytes1 > kjf::kMaxBytes) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 32 bytes");
  memset(info_format, 0, sizeof *info_format);
  uint32_t n;
  bool paired;
  int rc;
  if ((rc = classify_text_device(ctx, t, text1, bytes1, text2, bytes2, fastq, keep_names, rec_cap, info_parse, &n, &paired))) return rc;
  if ((rc = ensure(ctx->fmt_out, out_cap + 64))) return rc;
  if ((rc = ensure(ctx->fmt_info, sizeof(Info)))) return rc;
  if ((rc = format_staged(ctx, n, paired ? 1 : 0, bytes1, names, drop, out_text, out_cap, info_format))) return rc;
  if (info_format->overflow) return fail(KAIJU_GPU_ERR_ARG, "the output text needs more than out_cap bytes");
  return KAIJU_GPU_OK;
}

extern "C" int kaiju_gpu_format_compact(kaiju_gpu_ctx *ctx, const kaiju_gpu_compact *recs, const uint64_t *off, uint32_t n, int paired,
                                        const char *text1, uint64_t bytes1, const kaiju_gpu_name_span *names, char *out, uint64_t out_cap,
                                        kaiju_gpu_format_info *info) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format()) return rc;
  if (!ctx || !info || (n && (!recs || !off || !names)) || (!text1 && bytes1) || (!out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (bytes1 > kjf::kMaxBytes || n > kjf::kMaxRecords) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 32 bytes, a batch below 2^31 records");
  KJ_HIP(hipSetDevice(ctx->ix->device));
  if (int rc = format_stage(ctx, recs, off, n, text1, bytes1, names, out_cap, sizeof(kaiju_gpu_format_info))) return rc;
  return format_staged(ctx, n, paired, bytes1, nullptr, 0, out, out_cap, info);
  });
}

extern "C" int kaiju_gpu_classify_text_to_text(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const char *text1, uint64_t bytes1,
                                               const char *text2, uint64_t bytes2, int fastq, int keep_names, uint32_t rec_cap,
                                               char *out_text, uint64_t out_cap, kaiju_gpu_parse_info *info_parse,
                                               kaiju_gpu_format_info *info_format) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format()) return rc;
  if (!ctx || !t || !info_format || (!out_text && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  return text_to_text(ctx, t, text1, bytes1, text2, bytes2, fastq, keep_names, rec_cap, nullptr, 0, out_text, out_cap, info_parse, info_format);
  });
}

// ---- the output lines with taxon names on the device (format_names.hip) ------------------------------------------
static int no_format_names() { return kj_fn_launch && kaiju_gpu_taxon_names_max_annotation ? KAIJU_GPU_OK : fail(KAIJU_GPU_ERR_UNSUPPORTED, "this library was linked without format_names.hip"); }
extern "C" uint64_t kaiju_gpu_format_names_bound(uint64_t bytes1, uint32_t n, const kaiju_gpu_taxon_names *names) {
  const uint64_t most = names && kaiju_gpu_taxon_names_max_annotation ? kaiju_gpu_taxon_names_max_annotation(names) : 0;
  return bytes1 + (uint64_t)n * (kjn::kNamesExtra + most);
}
extern "C" int kaiju_gpu_format_names_device(kaiju_gpu_ctx *ctx, const kaiju_gpu_compact *d_recs, const uint64_t *d_off, uint32_t n, int paired,
                                             const void *d_text1, uint64_t bytes1, const kaiju_gpu_name_span *d_names,
                                             const kaiju_gpu_taxon_names *names, int drop_unclassified, void *d_out, uint64_t out_cap,
                                             kaiju_gpu_format_names_info *d_info, void *stream) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format_names()) return rc;
  if (!ctx) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  KJ_HIP(hipSetDevice(ctx->ix->device));
  return format_launch(ctx, stream ? static_cast<hipStream_t>(stream) : ctx->stream, d_recs, d_off, n, paired, d_text1, bytes1, d_names, names,
                       drop_unclassified, d_out, out_cap, d_info);
  });
}

extern "C" int kaiju_gpu_format_names(kaiju_gpu_ctx *ctx, const kaiju_gpu_compact *recs, const uint64_t *off, uint32_t n, int paired,
                                      const char *text1, uint64_t bytes1, const kaiju_gpu_name_span *names_spans,
                                      const kaiju_gpu_taxon_names *names, int drop_unclassified, char *out, uint64_t out_cap,
                                      kaiju_gpu_format_names_info *info) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format_names()) return rc;
  if (!ctx || !info || !names || (n && (!recs || !off || !names_spans)) || (!text1 && bytes1) || (!out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (bytes1 > kjf::kMaxBytes || n > kjf::kMaxRecords) return fail(KAIJU_GPU_ERR_ARG, "a block of text must be below 2^32 - 32 bytes, a batch below 2^31 records");
  KJ_HIP(hipSetDevice(ctx->ix->device));
  if (int rc = format_stage(ctx, recs, off, n, text1, bytes1, names_spans, out_cap, sizeof(kaiju_gpu_format_names_info))) return rc;
  return format_staged(ctx, n, paired, bytes1, names, drop_unclassified, out, out_cap, info);
  });
}

extern "C" int kaiju_gpu_classify_text_to_text_names(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const char *text1, uint64_t bytes1,
                                                     const char *text2, uint64_t bytes2, int fastq, int keep_names, uint32_t rec_cap,
                                                     const kaiju_gpu_taxon_names *names, int drop_unclassified, char *out_text, uint64_t out_cap,
                                                     kaiju_gpu_parse_info *info_parse, kaiju_gpu_format_names_info *info_format) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format_names()) return rc;
  if (!ctx || !t || !names || !info_format || (!out_text && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  return text_to_text(ctx, t, text1, bytes1, text2, bytes2, fastq, keep_names, rec_cap, names, drop_unclassified, out_text, out_cap, info_parse, info_format);
  });
}

// ---- the lines of kaiju -v on the device (format_verbose.hip) -----------------------------------------------------
int no_format_verbose() { return kj_fv_lengths && kaiju_accession_ranks ? KAIJU_GPU_OK : fail(KAIJU_GPU_ERR_UNSUPPORTED, "this library was linked without format_verbose.hip / accessions.cpp"); }

// ---- what the host entry points of kaiju -v and of kaijux / kaijup share (kjv::Job and kjq::Job name their inputs alike) ----
// the read names of n records to ctx->ing_text1 / ing_names, on the context's stream
static int stage_names(kaiju_gpu_ctx *ctx, const char *names_text, uint64_t names_bytes, const kaiju_gpu_name_span *names, uint32_t n) {
  int rc;
  if ((rc = ensure(ctx->ing_text1, names_bytes + 64))) return rc;
  if ((rc = ensure(ctx->ing_names, ((size_t)n + 1) * sizeof(kaiju_gpu_name_span)))) return rc;
  if (names_bytes) KJ_HIP(hipMemcpyAsync(ctx->ing_text1.p, names_text, names_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (n) KJ_HIP(hipMemcpyAsync(ctx->ing_names.p, names, (size_t)n * sizeof(kaiju_gpu_name_span), hipMemcpyHostToDevice, ctx->stream));
  return KAIJU_GPU_OK;
}
// the peptides of n records of kaiju_gpu_classify_batch_verbose_packed as the arrays of the device form: lengths, truncation
// marks, positions and the text to ctx->vb_tlen / fv_trunc / vb_pos / vb_packed; with_acc: the accessions to vb_nacc / vb_acc
static int stage_peptides(kaiju_gpu_ctx *ctx, const kaiju_gpu_verbose *vout, const uint64_t *text_pos, const char *text, uint64_t text_bytes,
                          uint32_t text_cap, uint32_t n, bool with_acc) {
  static_assert(kVbAcc == KAIJU_GPU_MAX_ACC, "rows of the accession array");
  std::vector<uint32_t> tlen((size_t)n + 1), trunc((size_t)n + 1), nacc, acc;
  if (with_acc) { nacc.resize((size_t)n + 1); acc.resize((size_t)n * kVbAcc + 1); }
  for (uint32_t r = 0; r < n; r++) {
    const kaiju_gpu_verbose &v = vout[r];
    tlen[r] = v.text_len; trunc[r] = v.truncated ? 1u : 0u;
    if (with_acc) { nacc[r] = v.n_acc; memcpy(&acc[(size_t)r * kVbAcc], v.acc_iseq, sizeof v.acc_iseq); }
    const uint64_t w = std::min(v.text_len, text_cap);
    if (text_pos[r] > text_bytes || w > text_bytes - text_pos[r]) return fail(KAIJU_GPU_ERR_ARG, "the peptides of a record lie outside the text");
  }
  int rc;
  if ((rc = ensure(ctx->vb_tlen, ((size_t)n + 1) * 4))) return rc;
  if ((rc = ensure(ctx->fv_trunc, ((size_t)n + 1) * 4))) return rc;
  if ((rc = ensure(ctx->vb_pos, ((size_t)n + 1) * 8 + 16))) return rc;
  if ((rc = ensure(ctx->vb_packed, text_bytes + 16))) return rc;
  if (with_acc && (rc = ensure(ctx->vb_nacc, ((size_t)n + 1) * 4))) return rc;
  if (with_acc && (rc = ensure(ctx->vb_acc, (size_t)n * kVbAcc * 4 + 16))) return rc;
  hipStream_t s = ctx->stream;
  // (the host arrays are pageable: the copies have left them when hipMemcpyAsync returns)
  if (text_bytes) KJ_HIP(hipMemcpyAsync(ctx->vb_packed.p, text, text_bytes, hipMemcpyHostToDevice, s));
  if (n) {
    KJ_HIP(hipMemcpyAsync(ctx->vb_tlen.p, tlen.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    KJ_HIP(hipMemcpyAsync(ctx->fv_trunc.p, trunc.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    KJ_HIP(hipMemcpyAsync(ctx->vb_pos.p, text_pos, (size_t)n * 8, hipMemcpyHostToDevice, s));
    if (with_acc) {
      KJ_HIP(hipMemcpyAsync(ctx->vb_nacc.p, nacc.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
      KJ_HIP(hipMemcpyAsync(ctx->vb_acc.p, acc.data(), (size_t)n * kVbAcc * 4, hipMemcpyHostToDevice, s));
    }
  }
  return KAIJU_GPU_OK;
}
// the staged buffers of the context as the inputs of a job: the records and read names ...
template <class Job>
static void bind_records(const kaiju_gpu_ctx *ctx, Job &J, uint64_t names_bytes) {
  J.hits = static_cast<const kaiju_gpu_hit *>(ctx->h_hits.p); J.off = static_cast<const uint64_t *>(ctx->h_off.p);
  if constexpr (std::is_same<Job, kjv::Job>::value) J.recs = static_cast<const kaiju_gpu_compact *>(ctx->h_compact.p);
  J.names_text = static_cast<const uint8_t *>(ctx->ing_text1.p); J.names_bytes = names_bytes;
  J.names = static_cast<const kaiju_gpu_name_span *>(ctx->ing_names.p);
}
// ... and the peptides (staged: from stage_peptides, with truncation marks; else what verbose_queue left on the device)
template <class Job>
static void bind_peptides(const kaiju_gpu_ctx *ctx, Job &J, uint32_t text_cap, bool staged) {
  if constexpr (std::is_same<Job, kjv::Job>::value) { J.n_acc = static_cast<const uint32_t *>(ctx->vb_nacc.p); J.acc_iseq = static_cast<const uint32_t *>(ctx->vb_acc.p); }
  J.text_pos = static_cast<const uint64_t *>(ctx->vb_pos.p); J.text_len = static_cast<const uint32_t *>(ctx->vb_tlen.p);
  J.trunc = staged ? static_cast<const uint32_t *>(ctx->fv_trunc.p) : nullptr;
  J.pep = static_cast<const uint8_t *>(ctx->vb_packed.p); J.text_cap = text_cap;
}
// Size first, then write, then fetch: behind the lengths pass of `lines` the one wait for the size of the text, room for it in
// ctx->fv_out and vb_host, write(total, &err) - the job's write pass into fv_out / fv_info -, and the text and *info on the host
template <class Write>
static int write_sized_text(kaiju_gpu_ctx *ctx, const kjl::Lines &lines, uint64_t bound, const char *mark, Write &&write, const char **text,
                            uint64_t *text_bytes, kaiju_gpu_format_verbose_info *info) {
  hipStream_t s = ctx->stream;
  uint64_t total = 0;
  KJ_HIP(hipMemcpyAsync(&total, lines.total, sizeof total, hipMemcpyDeviceToHost, s));
  KJ_HIP(hipStreamSynchronize(s));
  call_mark(mark);
  if (total > bound) return fail(KAIJU_GPU_ERR_HIP, "the format passes report an impossible size");
  int rc;
  if ((rc = ensure(ctx->fv_out, total + 64))) return rc;
  if (ctx->vb_host.size() < total) ctx->vb_host.resize((size_t)total);
  const char *err = "";
  if ((rc = write(total, &err))) return fail(rc, err);
  KJ_HIP(hipMemcpyAsync(info, ctx->fv_info.p, sizeof *info, hipMemcpyDeviceToHost, s));
  if (total) KJ_HIP(hipMemcpyAsync(ctx->vb_host.data(), ctx->fv_out.p, (size_t)total, hipMemcpyDeviceToHost, s));
  KJ_HIP(hipStreamSynchronize(s));
  if (info->text_bytes != total || info->overflow) return fail(KAIJU_GPU_ERR_HIP, "the format passes wrote another size than they announced");
  *text = reinterpret_cast<const char *>(ctx->vb_host.data());
  *text_bytes = total;
  return KAIJU_GPU_OK;
}

// the inputs of the passes that come from the context and its index; everything else is the caller's
static int fv_job(kaiju_gpu_ctx *ctx, int paired, kjv::Job &J) {
  if (ctx->ix->id_mode != KAIJU_GPU_IDS_TAXON) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "the lines of kaijux / kaijup are not made on the device");
  if (int rc = format_params(ctx, paired, J.P)) return rc;
  if (!index_accessions(ctx->ix, J)) return fail(KAIJU_GPU_ERR_ARG, "the index has no accession table on the device: call kaiju_gpu_index_upload_accessions() first");
  J.nseq = (uint32_t)ctx->ix->names.size();
  J.pw = static_cast<const double *>(ctx->fmt_pw.p);
  return KAIJU_GPU_OK;
}

extern "C" int kaiju_gpu_format_verbose_device(kaiju_gpu_ctx *ctx, const kaiju_gpu_hit *d_hits, const kaiju_gpu_compact *d_recs,
                                               const uint64_t *d_off, uint32_t n, int paired, const uint32_t *d_n_acc,
                                               const uint32_t *d_acc_iseq, const uint64_t *d_text_pos, const uint32_t *d_text_len,
                                               const void *d_pep, uint32_t text_cap, const void *d_names_text, uint64_t names_bytes,
                                               const kaiju_gpu_name_span *d_names, void *d_out, uint64_t out_cap,
                                               kaiju_gpu_format_verbose_info *d_info, void *stream) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format_verbose()) return rc;
  if (!ctx || !d_info || (!d_out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if ((uintptr_t)d_out & 15) return fail(KAIJU_GPU_ERR_ARG, "the output pointer must be 16-byte aligned");
  KJ_HIP(hipSetDevice(ctx->ix->device));
  kjv::Job J{};
  if (int rc = fv_job(ctx, paired, J)) return rc;
  J.hits = d_hits; J.recs = d_recs; J.off = d_off; J.n_acc = d_n_acc; J.acc_iseq = d_acc_iseq; J.text_pos = d_text_pos; J.text_len = d_text_len;
  J.pep = static_cast<const uint8_t *>(d_pep); J.text_cap = text_cap; J.names_text = static_cast<const uint8_t *>(d_names_text);
  J.names_bytes = names_bytes; J.names = d_names;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  const char *err = "";
  int rc = kj_fv_lengths(ctx->format_v, s, J, n, &err);
  if (rc) return fail(rc, err);
  rc = kj_fv_write(ctx->format_v, s, J, n, d_out, out_cap, d_info, &err);
  return rc ? fail(rc, err) : KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_format_verbose(kaiju_gpu_ctx *ctx, const kaiju_gpu_hit *hits, const kaiju_gpu_verbose *vout, const uint64_t *text_pos,
                                        const char *text, uint64_t text_bytes, uint32_t text_cap, const kaiju_gpu_compact *recs,
                                        const uint64_t *off, uint32_t n, int paired, const char *names_text, uint64_t names_bytes,
                                        const kaiju_gpu_name_span *names, char *out, uint64_t out_cap, kaiju_gpu_format_verbose_info *info) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format_verbose()) return rc;
  if (!ctx || !info || (n && (!hits || !vout || !text_pos || !recs || !off || !names)) || (!text && text_bytes) || (!names_text && names_bytes) ||
      (!out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (names_bytes > kjf::kMaxBytes || n > kjf::kMaxRecords) return fail(KAIJU_GPU_ERR_ARG, "the names must be below 2^32 - 32 bytes, a batch below 2^31 records");
  KJ_HIP(hipSetDevice(ctx->ix->device));
  kjv::Job J{};
  int rc;
  if ((rc = fv_job(ctx, paired, J))) return rc;
  if ((rc = stage_peptides(ctx, vout, text_pos, text, text_bytes, text_cap, n, true))) return rc;
  if ((rc = ensure(ctx->h_hits, ((size_t)n + 1) * sizeof(kaiju_gpu_hit)))) return rc;
  if ((rc = ensure(ctx->h_compact, ((size_t)n + 1) * sizeof(kaiju_gpu_compact)))) return rc;
  if ((rc = ensure(ctx->h_off, (2 * (size_t)n + 1) * 8))) return rc;
  if ((rc = stage_names(ctx, names_text, names_bytes, names, n))) return rc;
  if ((rc = ensure(ctx->fv_out, out_cap + 64))) return rc;
  if ((rc = ensure(ctx->fv_info, sizeof(kaiju_gpu_format_verbose_info)))) return rc;
  hipStream_t s = ctx->stream;
  if (n) {
    KJ_HIP(hipMemcpyAsync(ctx->h_hits.p, hits, (size_t)n * sizeof(kaiju_gpu_hit), hipMemcpyHostToDevice, s));
    KJ_HIP(hipMemcpyAsync(ctx->h_compact.p, recs, (size_t)n * sizeof(kaiju_gpu_compact), hipMemcpyHostToDevice, s));
    KJ_HIP(hipMemcpyAsync(ctx->h_off.p, off, (2 * (size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
  }
  bind_records(ctx, J, names_bytes);
  bind_peptides(ctx, J, text_cap, true);
  const char *err = "";
  rc = kj_fv_lengths(ctx->format_v, s, J, n, &err);
  if (rc == 0) rc = kj_fv_write(ctx->format_v, s, J, n, ctx->fv_out.p, out_cap, static_cast<kaiju_gpu_format_verbose_info *>(ctx->fv_info.p), &err);
  if (rc) { (void)hipStreamSynchronize(s); return fail(rc, err); }
  return format_download(s, ctx->format_v, ctx->fv_info, ctx->fv_out, out, out_cap, info);
  });
}

extern "C" int kaiju_gpu_classify_batch_verbose_text(kaiju_gpu_ctx *ctx, const kaiju_gpu_taxonomy *t, const char *seqs, const uint64_t *off,
                                                     uint32_t n_reads, int paired, const char *names_text, uint64_t names_bytes,
                                                     const kaiju_gpu_name_span *names, const char **text, uint64_t *text_bytes,
                                                     kaiju_gpu_format_verbose_info *info) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format_verbose()) return rc;
  if (!ctx || !t || !off || !text || !text_bytes || !info || (n_reads && !names) || (!names_text && names_bytes)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (t->device != ctx->ix->device) return fail(KAIJU_GPU_ERR_ARG, "taxonomy lives on another device");
  if (names_bytes > kjf::kMaxBytes || n_reads > kjf::kMaxRecords) return fail(KAIJU_GPU_ERR_ARG, "the names must be below 2^32 - 32 bytes, a batch below 2^31 records");
  *text = nullptr; *text_bytes = 0;
  memset(info, 0, sizeof *info);
  if (n_reads == 0) return KAIJU_GPU_OK;
  KJ_HIP(hipSetDevice(ctx->ix->device));
  kjv::Job J{};
  int rc;
  if ((rc = fv_job(ctx, paired, J))) return rc;
  if ((rc = stage_names(ctx, names_text, names_bytes, names, n_reads))) return rc;
  if ((rc = ensure(ctx->h_compact, ((size_t)n_reads + 1) * sizeof(kaiju_gpu_compact)))) return rc;
  if ((rc = ensure(ctx->fv_info, sizeof(kaiju_gpu_format_verbose_info)))) return rc;
  hipStream_t s = ctx->stream;
  if ((rc = verbose_queue(ctx, seqs, off, n_reads, paired))) return rc;
  if ((rc = launch_lca(s, t, static_cast<const kaiju_gpu_hit *>(ctx->h_hits.p), n_reads, static_cast<kaiju_gpu_compact *>(ctx->h_compact.p)))) return rc;
  bind_records(ctx, J, names_bytes);
  bind_peptides(ctx, J, ctx->vb_text_cap, false);
  const char *err = "";
  if ((rc = kj_fv_lengths(ctx->format_v, s, J, n_reads, &err))) return fail(rc, err);
  // (a line is its name and at most: "C\t" "\t" two numbers, 21 ids, 20 prefixes, the peptides, the tabs)
  return write_sized_text(ctx, ctx->format_v, names_bytes + (uint64_t)n_reads * (512 + 20ull * (kjv::kMaxPrefix + 1) + ctx->vb_text_cap),
                          "verbose text: size of the text on the host", [&](uint64_t total, const char **e) {
    return kj_fv_write(ctx->format_v, s, J, n_reads, ctx->fv_out.p, total, static_cast<kaiju_gpu_format_verbose_info *>(ctx->fv_info.p), e);
  }, text, text_bytes, info);
  });
}

// ---- the lines of kaijux / kaijup on the device (format_seq.hip) --------------------------------------------------
int no_format_seq() { return kj_fs_lengths ? KAIJU_GPU_OK : fail(KAIJU_GPU_ERR_UNSUPPORTED, "this library was linked without format_seq.hip"); }

// the inputs of the passes that come from the context and its index; everything else is the caller's
static int fs_job(kaiju_gpu_ctx *ctx, int paired, int u_rule, kjq::Job &J) {
  if (ctx->ix->id_mode != KAIJU_GPU_IDS_SEQUENCE) return fail(KAIJU_GPU_ERR_ARG, "the lines of kaijux / kaijup need an index loaded with KAIJU_GPU_IDS_SEQUENCE");
  if (u_rule != KAIJU_GPU_U_RULE_NUCLEOTIDE && u_rule != KAIJU_GPU_U_RULE_PROTEIN) return fail(KAIJU_GPU_ERR_ARG, "u_rule must be KAIJU_GPU_U_RULE_NUCLEOTIDE or KAIJU_GPU_U_RULE_PROTEIN");
  if (int rc = format_params(ctx, paired, J.P)) return rc;
  if (!index_seq_names(ctx->ix, J)) return fail(KAIJU_GPU_ERR_ARG, "the index has no sequence-name table on the device: call kaiju_gpu_index_upload_seq_names() first");
  J.nseq = (uint32_t)ctx->ix->names.size();
  J.pw = static_cast<const double *>(ctx->fmt_pw.p);
  J.u_rule = (uint32_t)u_rule;
  J.min_frag = ctx->params.min_fragment_length;
  J.min_score = ctx->params.min_score;
  J.greedy = ctx->params.mode == 0 ? 0u : 1u;
  return KAIJU_GPU_OK;
}

extern "C" int kaiju_gpu_format_seq_device(kaiju_gpu_ctx *ctx, const kaiju_gpu_hit *d_hits, const uint64_t *d_off, uint32_t n, int paired,
                                           int u_rule, const void *d_seqs, const uint64_t *d_text_pos, const uint32_t *d_text_len,
                                           const void *d_pep, uint32_t text_cap, const void *d_names_text, uint64_t names_bytes,
                                           const kaiju_gpu_name_span *d_names, void *d_out, uint64_t out_cap,
                                           kaiju_gpu_format_verbose_info *d_info, void *stream) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format_seq()) return rc;
  if (!ctx || !d_info || (!d_out && out_cap)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if ((uintptr_t)d_out & 15) return fail(KAIJU_GPU_ERR_ARG, "the output pointer must be 16-byte aligned");
  KJ_HIP(hipSetDevice(ctx->ix->device));
  kjq::Job J{};
  if (int rc = fs_job(ctx, paired, u_rule, J)) return rc;
  J.hits = d_hits; J.off = d_off; J.seqs = static_cast<const uint8_t *>(d_seqs);
  J.pep = static_cast<const uint8_t *>(d_pep);
  if (d_pep) { J.text_pos = d_text_pos; J.text_len = d_text_len; J.text_cap = text_cap; }
  J.names_text = static_cast<const uint8_t *>(d_names_text); J.names_bytes = names_bytes; J.names = d_names;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : ctx->stream;
  const char *err = "";
  int rc = kj_fs_lengths(ctx->format_s, s, J, n, &err);
  if (rc) return fail(rc, err);
  rc = kj_fs_write(ctx->format_s, s, J, n, d_out, out_cap, d_info, &err);
  return rc ? fail(rc, err) : KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_format_seq(kaiju_gpu_ctx *ctx, const kaiju_gpu_hit *hits, const uint64_t *off, uint32_t n, int paired, int u_rule,
                                    const char *seqs, const kaiju_gpu_verbose *vout, const uint64_t *text_pos, const char *text,
                                    uint64_t text_bytes, uint32_t text_cap, const char *names_text, uint64_t names_bytes,
                                    const kaiju_gpu_name_span *names, char *out, uint64_t out_cap, kaiju_gpu_format_verbose_info *info) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format_seq()) return rc;
  if (!ctx || !info || (n && (!hits || !off || !names)) || (n && text && (!vout || !text_pos)) || (!names_text && names_bytes) || (!out && out_cap))
    return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (names_bytes > kjf::kMaxBytes || n > kjf::kMaxRecords) return fail(KAIJU_GPU_ERR_ARG, "the names must be below 2^32 - 32 bytes, a batch below 2^31 records");
  KJ_HIP(hipSetDevice(ctx->ix->device));
  kjq::Job J{};
  int rc;
  if ((rc = fs_job(ctx, paired, u_rule, J))) return rc;
  const bool scan = u_rule == KAIJU_GPU_U_RULE_PROTEIN;
  uint64_t seq_bytes = 0;
  for (uint64_t i = 0; i < 2 * (uint64_t)n; i++) if (off[i + 1] < off[i]) return fail(KAIJU_GPU_ERR_ARG, "offsets must be non-decreasing");
  if (scan && n) { seq_bytes = off[2 * (uint64_t)n]; if (seq_bytes && !seqs) return fail(KAIJU_GPU_ERR_ARG, "seqs is NULL"); }
  if (text && (rc = stage_peptides(ctx, vout, text_pos, text, text_bytes, text_cap, n, false))) return rc;
  if ((rc = ensure(ctx->h_hits, ((size_t)n + 1) * sizeof(kaiju_gpu_hit)))) return rc;
  if ((rc = ensure(ctx->h_off, (2 * (size_t)n + 1) * 8))) return rc;
  if ((rc = ensure(ctx->h_seqs, seq_bytes + 64))) return rc;
  if ((rc = stage_names(ctx, names_text, names_bytes, names, n))) return rc;
  if ((rc = ensure(ctx->fv_out, out_cap + 64))) return rc;
  if ((rc = ensure(ctx->fv_info, sizeof(kaiju_gpu_format_verbose_info)))) return rc;
  hipStream_t s = ctx->stream;
  if (seq_bytes) KJ_HIP(hipMemcpyAsync(ctx->h_seqs.p, seqs, seq_bytes, hipMemcpyHostToDevice, s));
  {
    const uint64_t zero = 0;                             // (n = 0: off[0] is all there is)
    KJ_HIP(hipMemcpyAsync(ctx->h_off.p, n ? off : &zero, (2 * (size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
  }
  if (n) KJ_HIP(hipMemcpyAsync(ctx->h_hits.p, hits, (size_t)n * sizeof(kaiju_gpu_hit), hipMemcpyHostToDevice, s));
  bind_records(ctx, J, names_bytes);
  J.seqs = scan ? static_cast<const uint8_t *>(ctx->h_seqs.p) : nullptr;
  if (text) bind_peptides(ctx, J, text_cap, true);
  const char *err = "";
  rc = kj_fs_lengths(ctx->format_s, s, J, n, &err);
  if (rc == 0) rc = kj_fs_write(ctx->format_s, s, J, n, ctx->fv_out.p, out_cap, static_cast<kaiju_gpu_format_verbose_info *>(ctx->fv_info.p), &err);
  if (rc) { (void)hipStreamSynchronize(s); return fail(rc, err); }
  return format_download(s, ctx->format_s, ctx->fv_info, ctx->fv_out, out, out_cap, info);
  });
}

extern "C" int kaiju_gpu_classify_batch_seq_text(kaiju_gpu_ctx *ctx, const char *seqs, const uint64_t *off, uint32_t n_reads, int paired,
                                                 int verbose, int u_rule, const char *names_text, uint64_t names_bytes,
                                                 const kaiju_gpu_name_span *names, const char **text, uint64_t *text_bytes,
                                                 kaiju_gpu_format_verbose_info *info) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format_seq()) return rc;
  if (!ctx || !off || !text || !text_bytes || !info || (n_reads && !names) || (!names_text && names_bytes)) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (names_bytes > kjf::kMaxBytes || n_reads > kjf::kMaxRecords) return fail(KAIJU_GPU_ERR_ARG, "the names must be below 2^32 - 32 bytes, a batch below 2^31 records");
  *text = nullptr; *text_bytes = 0;
  memset(info, 0, sizeof *info);
  KJ_HIP(hipSetDevice(ctx->ix->device));
  kjq::Job J{};
  int rc;
  if ((rc = fs_job(ctx, paired, u_rule, J))) return rc;
  if (n_reads == 0) return KAIJU_GPU_OK;
  if ((rc = stage_names(ctx, names_text, names_bytes, names, n_reads))) return rc;
  if ((rc = ensure(ctx->fv_info, sizeof(kaiju_gpu_format_verbose_info)))) return rc;
  hipStream_t s = ctx->stream;
  uint32_t text_cap = 0;
  if (verbose) {
    if ((rc = verbose_queue(ctx, seqs, off, n_reads, paired))) return rc;
    text_cap = ctx->vb_text_cap;
    bind_peptides(ctx, J, text_cap, false);
  } else if ((rc = classify_host_buffers(ctx, seqs, off, n_reads, paired))) return rc;
  bind_records(ctx, J, names_bytes);
  J.seqs = static_cast<const uint8_t *>(ctx->h_seqs.p);
  const char *err = "";
  if ((rc = kj_fs_lengths(ctx->format_s, s, J, n_reads, &err))) return fail(rc, err);
  // (a line is its name and at most: "C\t" "\t" a number, 21 names with their commas, the peptides, two tabs, "\n")
  return write_sized_text(ctx, ctx->format_s, names_bytes + (uint64_t)n_reads * (64 + (uint64_t)kjq::kMaxIds * ((uint64_t)ctx->ix->sn_max + 1) + text_cap),
                          "seq text: size of the text on the host", [&](uint64_t total, const char **e) {
    return kj_fs_write(ctx->format_s, s, J, n_reads, ctx->fv_out.p, total, static_cast<kaiju_gpu_format_verbose_info *>(ctx->fv_info.p), e);
  }, text, text_bytes, info);
  });
}
