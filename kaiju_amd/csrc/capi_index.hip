// capi_index.hip - the index half of the C-ABI (include/kaiju_gpu.h): loading an index from a .fmi or an image file into HBM
// (streaming, the arrays built on the device), its digest, layout and read-back, and the two name tables that the formatters of
// kaiju -v and kaijux / kaijup read (accessions, sequence names).  capi_internal.h holds struct kaiju_gpu_index.
//
// Kernels: k_kmer_extend / k_kmer_extend_wide / k_kline_build (k-mer table), k_suffix_walk ... k_seq_walk_fill (row -> sequence
// tables and the text arrays), k_digest.
#include <fcntl.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <future>
#include <memory>
#include <mutex>
#include <thread>

#include "capi_internal.h"
#include "fmi_stream.h"
#include "host_index.h"
#include "host_tables.h"
#include "kj_rowtax_plan.h"
#include "kj_format_verbose.h"
#include "kj_format_seq.h"
// (variant libraries may be linked without accessions.cpp: capi_text.hip's no_format_verbose() says so first)
extern "C" __attribute__((weak)) decltype(kaiju_accession_ranks) kaiju_accession_ranks;

using namespace kj;

// Index load: the k-mer table one letter deeper.  child[idx * 20 + c - 1] = UpdateSI(parent[idx], c)
// (bwt.c:160-173) for all 20 letters from the two rank blocks at the ends of the parent's interval;
// empty intervals stay {0, 0}.  One thread per parent, 160 contiguous bytes of children each.
__global__ void __launch_bounds__(256)
k_kmer_extend(const RankBlock64 *__restrict__ blk, const uint2 *__restrict__ parent, uint2 *__restrict__ child,
              uint64_t n_parent) {
  for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < n_parent; idx += (uint64_t)gridDim.x * 256) {
    const uint2 e = parent[idx];
    uint32_t out[40];
#pragma unroll
    for (int x = 0; x < 40; x++) out[x] = 0;
    if (e.y != 0) {
      const uint32_t lo = e.x, hi = e.x + e.y;
      const RankBlock64 &A = blk[lo >> 6], &B = blk[hi >> 6];
      const uint64_t lowA = (1ull << (lo & 63u)) - 1ull, lowB = (1ull << (hi & 63u)) - 1ull;
#pragma unroll
      for (int c = 1; c <= 20; c++) {
        uint64_t ma = lowA, mb = lowB;
#pragma unroll
        for (int bit = 0; bit < 5; bit++) {
          ma &= ((c >> bit) & 1) ? A.plane[bit] : ~A.plane[bit];
          mb &= ((c >> bit) & 1) ? B.plane[bit] : ~B.plane[bit];
        }
        const uint32_t ra = A.cnt[c - 1] + (uint32_t)__popcll(ma), rb = B.cnt[c - 1] + (uint32_t)__popcll(mb);
        if (ra < rb) { out[2 * (c - 1)] = ra; out[2 * (c - 1) + 1] = rb - ra; }
      }
    }
    uint4 *dst = reinterpret_cast<uint4 *>(child + idx * 20);
#pragma unroll
    for (int x = 0; x < 10; x++) dst[x] = make_uint4(out[4 * x], out[4 * x + 1], out[4 * x + 2], out[4 * x + 3]);
  }
}

// Index load, narrow indexes: the k-mer LINES of the table just grown (kj_core.h: DevIndex::kline, kline_build_one): one
// thread per line - twenty entries gathered with a stride of 20^(k-1) (coalesced over the threads), twenty consecutive ones
// for the presence bits, the BWT letter of every one-row interval from its rank block.
__global__ void __launch_bounds__(256)
k_kline_build(DevIndex ix, uint32_t k, uint64_t n_lines, uint8_t *__restrict__ lines) {
  for (uint64_t code = (uint64_t)blockIdx.x * 256 + threadIdx.x; code < n_lines; code += (uint64_t)gridDim.x * 256)
    kline_build_one(ix, k, code, lines + code * kKLineBytes);
}

// Index load, narrow indexes with room to spare: the database text and the full suffix array for the text verification of the
// MEM lane (kj_core.h: DevIndex::sa_full / text).  k_suffix_walk: (sequence, offset) of the suffix of every row by the
// reference's own walk (suffix_of_row = get_suffix, bwt.c:105-121); k_seq_lens: a sequence's length = the offset of its
// terminator suffix (rows 0 .. nseq-1); k_text_build: row r's suffix lies at g = off[sequence] + 1 + offset, and the letter
// in front of it is the row's BWT letter.
__global__ void __launch_bounds__(256)
k_suffix_walk(DevIndex ix, const uint32_t *__restrict__ smp_pos, uint32_t *__restrict__ row_seq, uint32_t *__restrict__ row_pos, uint32_t *bad,
              uint32_t *__restrict__ beyond_rows) {
  // bad[0]: a row could not be resolved; bad[1]: number of rows whose walk passed the missing sample of an index with the
  // reference's short sample array (beyond_rows[0 .. kBeyondRowsMax): those rows - k_rows_beyond unsets their sequence)
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < ix.bwtlen; r += (uint64_t)gridDim.x * 256) {
    uint32_t sq = 0, ps = 0;
    bool by = false;
    if (!suffix_of_row(ix, smp_pos, r, sq, ps, &by) || sq >= ix.nseq) { atomicOr(bad, 1u); sq = 0; ps = 0; }
    if (by) { const uint32_t at = atomicAdd(bad + 1, 1u); if (at < kBeyondRowsMax) beyond_rows[at] = (uint32_t)r; }
    row_seq[r] = sq; row_pos[r] = ps;
  }
}
__global__ void __launch_bounds__(256)
k_rows_beyond(const uint32_t *__restrict__ beyond_rows, uint32_t n, uint32_t *__restrict__ row_seq) {
  const uint32_t x = blockIdx.x * 256 + threadIdx.x;
  if (x < n) row_seq[beyond_rows[x]] = 0xffffffffu;          // a locate of that row finds no sequence (the reference reads out of bounds there)
}
// row -> sequence becomes row -> dense taxon index (DevIndex::row_tax), in place; out[x] = src[idx[x]] (the text positions of the
// few rows behind the missing sample)
__global__ void __launch_bounds__(256)
k_row_tax(uint32_t *__restrict__ row_seq, uint64_t n, const uint32_t *__restrict__ seq_dense, uint32_t nseq) {
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256) {
    const uint32_t q = row_seq[r];
    row_seq[r] = q < nseq ? seq_dense[q] : 0xffffffffu;
  }
}
__global__ void __launch_bounds__(256)
k_gather_u32(const uint32_t *__restrict__ src, const uint32_t *__restrict__ idx, uint32_t n, uint32_t *__restrict__ out) {
  const uint32_t x = blockIdx.x * 256 + threadIdx.x;
  if (x < n) out[x] = src[idx[x]];
}
__global__ void __launch_bounds__(256)
k_seq_lens(uint32_t nseq, const uint32_t *__restrict__ row_seq, const uint32_t *__restrict__ row_pos, uint32_t *__restrict__ len) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r < nseq) len[row_seq[r]] = row_pos[r];
}
__global__ void __launch_bounds__(256)
k_text_build(DevIndex ix, const uint32_t *__restrict__ row_seq, const uint32_t *__restrict__ row_pos, const uint32_t *__restrict__ off,
             uint32_t *__restrict__ sa_full, uint8_t *__restrict__ text) {
  for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < ix.bwtlen; r += (uint64_t)gridDim.x * 256) {
    const uint32_t g = off[row_seq[r]] + 1u + row_pos[r];
    sa_full[r] = g;
    text[g - 1u] = (uint8_t)symbol_at(ix, r);
  }
}

// Index load, indexes with 64-bit positions that leave room: the database text and the text position of every 2^tv_shift-th
// row (DevIndex::sa_tpos5), by walking every sequence from its terminator row (seq_walk_len / seq_walk_fill, kj_core.h).  A lane
// that has finished a sequence takes the next one (sequences are 30 .. 30 000 letters long: a wave of 64 whole walks would wait
// for its longest), one LF step per loop iteration.
__global__ void __launch_bounds__(256)
k_seq_walk_len(DevIndex ix, uint32_t *next, uint32_t *__restrict__ t_seq, uint32_t *__restrict__ len, uint32_t *bad) {
  uint64_t k = 0, n = 0;
  uint32_t t = 0;
  bool active = false;
  for (;;) {
    if (!active) {
      t = atomicAdd(next, 1u);
      if (t >= ix.nseq) break;
      k = t; n = 0; active = true;
    }
    const uint32_t c = symbol_at(ix, k);
    // (no sequence is longer than the text, and its length must fit the 32 bits of len[]: a damaged image ends here - bad is set
    //  below - instead of spinning for billions of LF steps)
    if (c == 0 || n >= 0xfffffff0ull || n > ix.bwtlen) {
      const uint32_t q = c == 0 ? (uint32_t)rank_term(ix, k) : 0xffffffffu;
      if (q >= ix.nseq) { atomicOr(bad, 1u); t_seq[t] = 0; }
      else { t_seq[t] = q; len[q] = (uint32_t)n; }
      active = false;
    } else { k = rank_c(ix, c, k); n++; }
  }
}
__global__ void __launch_bounds__(256)
k_seq_walk_fill(DevIndex ix, uint32_t *next, const uint32_t *__restrict__ t_seq, const uint32_t *__restrict__ len, const uint64_t *__restrict__ off,
                uint8_t *__restrict__ text, uint8_t *__restrict__ tpos5, uint32_t tv_shift,
                uint32_t *__restrict__ row_tax, const uint32_t *__restrict__ seq_dense, uint32_t rt_shift) {
  // text / tpos5 (both or neither) and row_tax are optional: the walk fills what the index had room for
  // (rt_shift: row_tax is the table of every 2^rt_shift-th row, DevIndex::row_tax_s; 0 = of every row)
  const uint64_t tvm = (1ull << tv_shift) - 1ull, rtm = (1ull << rt_shift) - 1ull;
  uint64_t k = 0, g = 0, left = 0;
  uint32_t dq = 0xffffffffu;
  bool active = false;
  for (;;) {
    if (!active) {
      const uint32_t t = atomicAdd(next, 1u);
      if (t >= ix.nseq) break;
      const uint32_t q = t_seq[t];
      k = t; g = off[(size_t)q + 1]; left = (uint64_t)len[q] + 1; active = true;
      if (row_tax) dq = seq_dense[q];
    }
    if (row_tax && (k & rtm) == 0) row_tax[k >> rt_shift] = dq;
    const uint32_t c = symbol_at(ix, k);
    if (text) {
      if ((k & tvm) == 0) put_tpos5(tpos5, k >> tv_shift, g);
      text[g - 1] = (uint8_t)c;
    }
    if (c == 0 || --left == 0) active = false;
    else { k = rank_c(ix, c, k); g--; }
  }
}

// the same for indexes with 64-bit positions: 16-byte entries {lo, len}, counts relative to mb_base
__global__ void __launch_bounds__(256)
k_kmer_extend_wide(const RankBlock64 *__restrict__ blk, const uint64_t *__restrict__ mb_base, uint32_t mb_shift,
                   const ulonglong2 *__restrict__ parent, ulonglong2 *__restrict__ child, uint64_t n_parent) {
  for (uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x; idx < n_parent; idx += (uint64_t)gridDim.x * 256) {
    const ulonglong2 e = parent[idx];
    ulonglong2 *dst = child + idx * 20;
    if (e.y == 0) {
      for (int c = 0; c < 20; c++) dst[c] = make_ulonglong2(0, 0);
      continue;
    }
    const uint64_t lo = e.x, hi = e.x + e.y;
    const RankBlock64 &A = blk[lo >> 6], &B = blk[hi >> 6];
    const uint64_t *ma0 = mb_base + (lo >> mb_shift) * 20, *mb0 = mb_base + (hi >> mb_shift) * 20;
    const uint64_t lowA = (1ull << (lo & 63u)) - 1ull, lowB = (1ull << (hi & 63u)) - 1ull;
#pragma unroll
    for (int c = 1; c <= 20; c++) {
      uint64_t ma = lowA, mb = lowB;
#pragma unroll
      for (int bit = 0; bit < 5; bit++) {
        ma &= ((c >> bit) & 1) ? A.plane[bit] : ~A.plane[bit];
        mb &= ((c >> bit) & 1) ? B.plane[bit] : ~B.plane[bit];
      }
      const uint64_t ra = ma0[c - 1] + A.cnt[c - 1] + (uint64_t)__popcll(ma), rb = mb0[c - 1] + B.cnt[c - 1] + (uint64_t)__popcll(mb);
      dst[c - 1] = ra < rb ? make_ulonglong2(ra, rb - ra) : make_ulonglong2(0, 0);
    }
  }
}


// KAIJU_GPU_LOAD_TIMES=1: wall time of the phases of an index load / a context creation, on stderr
struct LoadClock {
  bool on;
  double t0, tl;
  static double now() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
  LoadClock() : on(getenv("KAIJU_GPU_LOAD_TIMES") != nullptr), t0(now()), tl(t0) {}
  void mark(const char *what) {
    if (!on) return;
    const double t = now();
    fprintf(stderr, "[kaiju_gpu load] %-34s %8.1f ms (at %8.1f ms)\n", what, (t - tl) * 1e3, (t - t0) * 1e3);
    tl = t;
  }
};

template <class T, class A>
static int upload(kaiju_gpu_index *ix, const std::vector<T, A> &v, const T **dst) {
  void *p = nullptr;
  const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16) + 32;   // slack: 16-byte loads of 8-byte entries
  KJ_HIP(hipMalloc(&p, bytes));
  ix->allocs.push_back(p);
  if (!v.empty()) KJ_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *dst = static_cast<const T *>(p);
  return 0;
}

// An array that was left in its image file (PackedIndex::lazy): file -> page-locked pieces -> HBM, two pieces in flight (the
// readers fill one while the other is on its way to the device), never a host copy of the whole array - a refseq-class image
// is 150 GB and eight ranks of a node load it side by side (the reference maps the whole .fmi into every process:
// readIndexes bwt/bwt.c:78-88).  KAIJU_GPU_STREAM_PIECE_MB sets the piece size (default 256; tests use 1).
struct ImageStreamer {
  int fd = -1;
  size_t piece = 0;
  void *buf[2] = {nullptr, nullptr};
  hipStream_t stream = nullptr;
  hipEvent_t done[2] = {nullptr, nullptr};
  uint64_t bytes_streamed = 0;
  double t_read = 0, t_total = 0;
  ~ImageStreamer() {
    if (fd >= 0) close(fd);
    for (int k = 0; k < 2; k++) { if (buf[k]) (void)hipHostFree(buf[k]); if (done[k]) (void)hipEventDestroy(done[k]); }
    if (stream) (void)hipStreamDestroy(stream);
  }
  int open_file(const std::string &path) {
    if (fd >= 0) return 0;
    fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return fail(KAIJU_GPU_ERR_IO, "cannot open " + path);
    size_t mb = 256;
    if (const char *e = getenv("KAIJU_GPU_STREAM_PIECE_MB")) { const long v = atol(e); if (v >= 1 && v <= 4096) mb = (size_t)v; }
    piece = mb << 20;
    if (const char *e = getenv("KAIJU_GPU_STREAM_PIECE_KB")) { const long v = atol(e); if (v >= 4 && v <= (4096L << 10)) piece = (size_t)v << 10; }   // (tests)
    for (int k = 0; k < 2; k++) {
      KJ_HIP(hipHostMalloc(&buf[k], piece, hipHostMallocDefault));
      KJ_HIP(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
    }
    KJ_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return 0;
  }
  // bytes [off, off + n) of the file to device memory at dst
  int run(uint64_t off, uint64_t n, void *dst) {
    const double t0 = LoadClock::now();
    const unsigned nthreads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    bool used[2] = {false, false};
    uint64_t at = 0;
    for (int k = 0; at < n; k ^= 1) {
      const size_t len = (size_t)std::min<uint64_t>(piece, n - at);
      if (used[k]) KJ_HIP(hipEventSynchronize(done[k]));               // the copy out of this buffer has finished
      const double tr = LoadClock::now();
      std::atomic<bool> ok{true};
      const size_t sub = std::max<size_t>((len + nthreads - 1) / nthreads, std::min<size_t>(1u << 20, std::max<size_t>(piece / 4, 4096)));
      std::vector<std::thread> th;
      for (size_t b = 0; b < len; b += sub) {
        const size_t e = std::min(len, b + sub);
        th.emplace_back([&, b, e]() {
          size_t q = b;
          uint8_t *d = static_cast<uint8_t *>(buf[k]);
          while (q < e) { const ssize_t r = pread(fd, d + q, e - q, (off_t)(off + at + q)); if (r <= 0) { ok = false; return; } q += (size_t)r; }
        });
      }
      for (auto &x : th) x.join();
      t_read += LoadClock::now() - tr;
      if (!ok.load()) return fail(KAIJU_GPU_ERR_IO, "short read from the index image");
      KJ_HIP(hipMemcpyAsync(static_cast<uint8_t *>(dst) + at, buf[k], len, hipMemcpyHostToDevice, stream));
      KJ_HIP(hipEventRecord(done[k], stream));
      used[k] = true;
      at += len;
    }
    KJ_HIP(hipStreamSynchronize(stream));
    bytes_streamed += n;
    t_total += LoadClock::now() - t0;
    return 0;
  }
};

// a host vector, or - when it is empty and the image reader left the array in its file - the file's bytes
template <class T, class A>
static int upload_arr(kaiju_gpu_index *ix, ImageStreamer &is, const std::string &path, const std::vector<T, A> &v, const LazyArr &l, const T **dst) {
  if (!v.empty() || l.n == 0) return upload(ix, v, dst);
  int rc = is.open_file(path);
  if (rc) return rc;
  void *p = nullptr;
  KJ_HIP(hipMalloc(&p, l.n * sizeof(T) + 32));
  ix->allocs.push_back(p);
  if ((rc = is.run(l.off, l.n * sizeof(T), p))) return rc;
  *dst = static_cast<const T *>(p);
  return 0;
}

static int index_from_packed(PackedIndex &pk, int device_id, kaiju_gpu_index **out, bool keep_packed = false);
static thread_local int tl_id_mode = 0;     // kaiju_gpu_index_load_ex: 1 = hits collect sequence numbers

// The first HIP call of a process starts the runtime (about 0.15 s on an MI355X host); reading and packing an index needs
// no device, so the check for one runs beside it.  Its verdict still comes first: without a device the load fails with
// KAIJU_GPU_ERR_NO_DEVICE whatever the file looks like.
static std::future<int> device_check_async(int device_id) {
  return std::async(std::launch::async, [device_id]() -> int {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return KAIJU_GPU_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= ndev) return KAIJU_GPU_ERR_ARG;
    if (hipSetDevice(device_id) != hipSuccess || hipFree(nullptr) != hipSuccess) return KAIJU_GPU_ERR_HIP;
    return KAIJU_GPU_OK;
  });
}
static int device_check_result(std::future<int> &f) {
  const int rc = f.get();
  if (rc == KAIJU_GPU_ERR_NO_DEVICE) return fail(rc, "hipGetDeviceCount found no device");
  if (rc == KAIJU_GPU_ERR_ARG) return fail(rc, "device_id out of range");
  if (rc) return fail(rc, "the HIP runtime did not start on that device");
  return KAIJU_GPU_OK;
}

static int index_from_view(const HostIndexView &v, int device_id, kaiju_gpu_index **out, std::future<int> *dev_started = nullptr) {
  if (!out) return fail(KAIJU_GPU_ERR_ARG, "out is NULL");
  *out = nullptr;
  std::future<int> own;
  if (!dev_started) { own = device_check_async(device_id); dev_started = &own; }
  std::string msg;
  PackedIndex pk;
  LoadClock lc;
  int rc = pk.build(v, msg);
  lc.mark("pack (host)");
  const int drc = device_check_result(*dev_started);
  lc.mark("wait for the HIP runtime");
  if (drc) return drc;
  if (rc) return fail(rc, msg);
  return index_from_packed(pk, device_id, out);
}

// upload of the packed arrays (from a freshly packed .fmi or from an image file)
static int index_from_packed(PackedIndex &pk, int device_id, kaiju_gpu_index **out, bool keep_packed) {
  std::string msg;
  int rc;
  LoadClock lc;
  if (tl_id_mode == 1) pk.to_sequence_ids();
  std::unique_ptr<kaiju_gpu_index> ix(new kaiju_gpu_index());
  ix->device = device_id;
  ix->id_mode = tl_id_mode;
  rc = build_const_tables(pk.trans, ix->ct_host, msg);
  if (rc) return fail(rc, msg);
  std::vector<double> lnfact;
  rc = build_seg_tables(lnfact, ix->st, msg);
  if (rc) return fail(rc, msg);
  lc.mark("host tables");
  KJ_HIP(hipSetDevice(device_id));
  DevIndex &d = ix->dev;
  // what goes to HBM per index row: rank blocks 2 B, SA sample (e = 3) 0.5 B of sequence numbers and, on a
  // narrow index, 1 B of taxon ids
  ImageStreamer is;
  const std::string &ipath = pk.lazy.path;
  const bool streamed = !pk.stream.path.empty();       // a .fmi whose BWT and samples are still in the file (fmi_stream.h)
  const uint32_t *d_stream_sa_pos = nullptr;
  if ((rc = upload(ix.get(), pk.seq_taxid, &d.seq_taxid))) return rc;
  if ((rc = upload(ix.get(), pk.seq_valid, &d.seq_valid))) return rc;
  d.mb_base = nullptr; d.mb_shift = pk.mb_shift;
  d.sa_taxid = nullptr;
  if (streamed) {
    // file -> page-locked pieces -> HBM, packed by kernels: no host copy of bwt[] / sa[], no packed arrays on the host
    FmiStreamResult sr;
    if ((rc = fmi_stream_to_device(pk.stream, pk, d.seq_taxid, d.seq_valid, sr, msg))) return fail(rc, msg);
    for (void *p : {(void *)sr.blocks64, (void *)sr.mb_base, (void *)sr.sa_iseq, (void *)sr.sa_taxid, (void *)sr.term_pos}) if (p) ix->allocs.push_back(p);
    d.blocks64 = sr.blocks64; d.mb_base = sr.mb_base; d.sa_iseq = sr.sa_iseq; d.sa_taxid = sr.sa_taxid; d.term_pos = sr.term_pos;
    d_stream_sa_pos = sr.sa_pos;                       // (freed behind the text builder below)
    if (sr.sa_pos) ix->allocs.push_back(sr.sa_pos);
    memcpy(pk.C, sr.C, sizeof pk.C);
    if (sr.mb_base) {                                  // (a few KB; kept on the host for the footprint and kaiju_gpu_index_load_devices)
      pk.mb_base.resize((size_t)((pk.bwtlen >> pk.mb_shift) + 1) * 20);
      KJ_HIP(hipMemcpy(pk.mb_base.data(), sr.mb_base, pk.mb_base.size() * 8, hipMemcpyDeviceToHost));
    }
    if (lc.on)
      fprintf(stderr, "[kaiju_gpu load]   streamed from the .fmi: %.2f GB in %.2f s (%.1f GB/s; %.2f s of it reading pieces into page-locked "
                      "memory, pieces of %.1f MB), packed on the device\n", sr.bytes_streamed * 1e-9, sr.seconds, sr.bytes_streamed * 1e-9 / std::max(sr.seconds, 1e-9),
              sr.seconds_reading, sr.piece / 1048576.0);
  } else {
    if ((rc = upload_arr(ix.get(), is, ipath, pk.blocks64, pk.lazy.blocks64, &d.blocks64))) return rc;
    if (!pk.mb_base.empty() && (rc = upload(ix.get(), pk.mb_base, &d.mb_base))) return rc;
    if (!pk.sa_taxid.empty() && (rc = upload(ix.get(), pk.sa_taxid, &d.sa_taxid))) return rc;
    if ((rc = upload_arr(ix.get(), is, ipath, pk.sa_iseq, pk.lazy.sa_iseq, &d.sa_iseq))) return rc;
    if ((rc = upload_arr(ix.get(), is, ipath, pk.term_pos, pk.lazy.term_pos, &d.term_pos))) return rc;
  }
  const double *dl = nullptr;
  if ((rc = upload(ix.get(), lnfact, &dl))) return rc;
  ix->st.lnfact = dl;
  // the window-probability table of s_Trim: no index data (not in kj::index_arrays, the digest or the image).
  // KAIJU_GPU_SEG_TABLE=0: the SEG kernels compute every window directly
  uint64_t seg_tab_bytes = 0;
  {
    const SegProbTable &pt = seg_prob_table();
    const std::vector<uint64_t> keyw(pt.T, pt.T + kSegKeyWords);
    if ((rc = upload(ix.get(), pt.slots, &ix->d_ptab))) return rc;
    if ((rc = upload(ix.get(), keyw, &ix->d_ptab_T))) return rc;
    seg_tab_bytes = pt.slots.size() * sizeof(SegProbEntry) + keyw.size() * 8;
    const char *e = getenv("KAIJU_GPU_SEG_TABLE");
    const bool off = ix->st.ptab == nullptr || (e && atoi(e) == 0);
    ix->st.ptab = off ? nullptr : ix->d_ptab;
    ix->st.ptab_T = off ? nullptr : ix->d_ptab_T;
  }
  {
    std::vector<Stage1Tables> s1(1);
    build_stage1_tables(ix->ct_host, ix->st, s1[0]);
    const Stage1Tables *d1 = nullptr;
    if ((rc = upload(ix.get(), s1, &d1))) return rc;
    ix->d_s1 = d1;
  }
  std::vector<ConstTables> ctv(1, ix->ct_host);
  const ConstTables *dct = nullptr;
  if ((rc = upload(ix.get(), ctv, &dct))) return rc;
  ix->d_ct = const_cast<ConstTables *>(dct);
  for (int a = 0; a < 22; a++) d.C[a] = pk.C[a];
  d.bwtlen = pk.bwtlen; d.n_sa = pk.n_sa; d.sa_skip = pk.sa_skip; d.nseq = pk.nseq; d.chpt_exp = pk.chpt_exp;
  d.kmer32 = nullptr; d.kmer64 = nullptr; d.kmer_k = pk.kmer_k; d.kline = nullptr; d.kline_k = 0;
  const uint64_t n_kmer32 = PackedIndex::count(pk.kmer32, pk.lazy.kmer32), n_kmer64 = PackedIndex::count(pk.kmer64, pk.lazy.kmer64);
  uint64_t kmer_bytes = 0;
  // the depth the HOST packer builds (PackedIndex::build: 5, KAIJU_GPU_KMER up to 6); a streamed .fmi has no rank blocks on the
  // host: its table starts on the device with the twenty one-letter intervals of InitialSI (bwt.c:146-152) and grows from there
  constexpr uint32_t kKmerResidentK = 5;          // depth of the table a narrow index keeps next to its k-mer lines
  void *kmer5 = nullptr;
  // (the five-letter level is in nobody's list while the deeper levels grow: an early return below must not leak it)
  struct FreeOnExit { void *&p; ~FreeOnExit() { if (p) (void)hipFree(p); } } kmer5_guard{kmer5};
  uint32_t host_k = pk.kmer_k;
  if (streamed && pk.alen == 21) {
    host_k = 5;
    if (const char *e = getenv("KAIJU_GPU_KMER")) { host_k = (uint32_t)atoi(e); if (host_k > 6) host_k = 6; }
    if (host_k < 2) host_k = 0;
    if (host_k) {
      if (!d.mb_base) {
        std::vector<uint2> k1(20);
        for (uint32_t c = 1; c <= 20; c++) { const uint64_t len = pk.C[c + 1] - pk.C[c]; k1[c - 1] = uint2{len ? (uint32_t)pk.C[c] : 0u, (uint32_t)len}; }
        if ((rc = upload(ix.get(), k1, &d.kmer32))) return rc;
      } else {
        std::vector<ulonglong2> k1(20);
        for (uint32_t c = 1; c <= 20; c++) { const uint64_t len = pk.C[c + 1] - pk.C[c]; k1[c - 1] = ulonglong2{len ? pk.C[c] : 0ull, len}; }
        if ((rc = upload(ix.get(), k1, &d.kmer64))) return rc;
      }
      d.kmer_k = 1;
    }
  }
  if (host_k) {
    if (streamed) {}
    else if (n_kmer32) { if ((rc = upload_arr(ix.get(), is, ipath, pk.kmer32, pk.lazy.kmer32, &d.kmer32))) return rc; }
    else if ((rc = upload_arr(ix.get(), is, ipath, pk.kmer64, pk.lazy.kmer64, &d.kmer64))) return rc;
    lc.mark("upload of the packed arrays");
    if (is.bytes_streamed && lc.on)
      fprintf(stderr, "[kaiju_gpu load]   streamed from the image file: %.2f GB in %.2f s (%.1f GB/s; %.2f s of it reading pieces into "
                      "page-locked memory, pieces of %zu MB)\n", is.bytes_streamed * 1e-9, is.t_total, is.bytes_streamed * 1e-9 / std::max(is.t_total, 1e-9),
              is.t_read, is.piece >> 20);
    // Deeper tables are grown on the device, one letter at a time.  Depth: KAIJU_GPU_KMER, or the
    // largest k <= 7 whose table (20^k entries of 8 bytes) has at most 8 entries per index row -
    // 10 GB for a viruses-size index, which is what 288 GB of HBM are for.
    uint32_t want = host_k;
    if (const char *e = getenv("KAIJU_GPU_KMER")) want = (uint32_t)atoi(e);
    else { uint64_t nn = 1; for (uint32_t q = 0; q < host_k; q++) nn *= 20; while (want < 7 && nn * 20 <= 8 * pk.bwtlen) { nn *= 20; want++; } }
    if (want > 7) want = 7;
    if (d.kmer32 && d.blocks64 && want > d.kmer_k) {
      uint64_t np = 1;
      for (uint32_t q = 0; q < d.kmer_k; q++) np *= 20;
      const uint2 *cur = d.kmer32;
      void *cur_alloc = ix->allocs.back();
      while (d.kmer_k < want) {
        void *child = nullptr;
        if (hipMalloc(&child, np * 20 * sizeof(uint2) + 64) != hipSuccess) { (void)hipGetLastError(); break; }   // keep the table we have
        const uint64_t blocks = std::min<uint64_t>((np + 255) / 256, 1u << 20);
        hipLaunchKernelGGL(k_kmer_extend, dim3((unsigned)blocks), dim3(256), 0, 0, d.blocks64, cur, static_cast<uint2 *>(child), np);
        KJ_HIP(hipGetLastError());
        KJ_HIP(hipDeviceSynchronize());
        // (the five-letter level stays: what remains resident once the lines of the deeper table exist, see below)
        if (d.kmer_k == kKmerResidentK && !d.mb_base && !getenv("KAIJU_GPU_KEEP_KMER_TABLE")) kmer5 = cur_alloc;
        else (void)hipFree(cur_alloc);
        ix->allocs.back() = child;
        cur_alloc = child; cur = static_cast<const uint2 *>(child);
        np *= 20; d.kmer_k++;
      }
      d.kmer32 = cur;
      kmer_bytes = np * sizeof(uint2) - n_kmer32 * sizeof(uint2);
    }
    d.kline = nullptr;
    if (d.kmer32 && d.blocks64 && !d.mb_base && d.kmer_k >= 2) {
      // the k-mer lines the second-generation lanes read (128 bytes per (k-1)-letter word; k = 7: 8.2 GB)
      uint64_t nl = 1;
      for (uint32_t q = 1; q < d.kmer_k; q++) nl *= 20;
      void *lines = nullptr;
      if (hipMalloc(&lines, nl * kKLineBytes + 256) == hipSuccess) {
        ix->allocs.push_back(lines);
        const uint64_t blocks = std::min<uint64_t>((nl + 255) / 256, 1u << 20);
        hipLaunchKernelGGL(k_kline_build, dim3((unsigned)blocks), dim3(256), 0, 0, d, d.kmer_k, nl, static_cast<uint8_t *>(lines));
        KJ_HIP(hipGetLastError());
        KJ_HIP(hipDeviceSynchronize());
        d.kline = static_cast<const uint8_t *>(lines);
        d.kline_k = d.kmer_k;
        kmer_bytes += nl * kKLineBytes;
        if (kmer5) {
          // The second-generation lanes read the LINES only; the table itself (20^7 entries: 10.2 GB on a viruses-size index,
          // half of its footprint) served the first-generation lanes - verbose output, the retry pass - which are as exact
          // with the five-letter level: that one stays (25.6 MB), the deep table goes
          ix->allocs.pop_back();                                        // (lines)
          (void)hipFree(ix->allocs.back());                             // (the deep table)
          ix->allocs.back() = kmer5;
          ix->allocs.push_back(lines);
          d.kmer32 = static_cast<const uint2 *>(kmer5); d.kmer_k = kKmerResidentK;
          kmer5 = nullptr;
        }
      } else (void)hipGetLastError();      // (no room: the lanes of the first generation serve, with the table)
    }
    if (kmer5) { (void)hipFree(kmer5); kmer5 = nullptr; }               // (no lines were built: the deep table stays as it is)
    if (d.kmer64 && d.blocks64 && d.mb_base && want > d.kmer_k) {
      uint64_t np = 1;
      for (uint32_t q = 0; q < d.kmer_k; q++) np *= 20;
      const ulonglong2 *cur = d.kmer64;
      void *cur_alloc = ix->allocs.back();
      while (d.kmer_k < want) {
        void *child = nullptr;
        if (hipMalloc(&child, np * 20 * sizeof(ulonglong2) + 64) != hipSuccess) { (void)hipGetLastError(); break; }
        const uint64_t blocks = std::min<uint64_t>((np + 255) / 256, 1u << 20);
        hipLaunchKernelGGL(k_kmer_extend_wide, dim3((unsigned)blocks), dim3(256), 0, 0, d.blocks64, d.mb_base, d.mb_shift, cur,
                           static_cast<ulonglong2 *>(child), np);
        KJ_HIP(hipGetLastError());
        KJ_HIP(hipDeviceSynchronize());
        (void)hipFree(cur_alloc);
        ix->allocs.back() = child;
        cur_alloc = child; cur = static_cast<const ulonglong2 *>(child);
        np *= 20; d.kmer_k++;
      }
      d.kmer64 = cur;
      kmer_bytes = np * sizeof(ulonglong2) - n_kmer64 * sizeof(ulonglong2);
    }
  }
  lc.mark("k-mer table (device)");
  // ---- text verification: the database text (1 B per row), the full suffix array and the sequence of every row (4 B per row
  //      each: 9 bytes per row in all, + 4 B per sequence for the text offsets; narrow indexes with room for it).  Room = twice
  //      the peak of the build (two temporaries of 4 B per row next to the arrays) plus what the classification contexts of
  //      two streams allocate later (scratch of the search lanes, peptides, fragment lists: up to ~4 GB for 10 M-read batches) -
  //      an index that does not leave that much goes without the text arrays rather than failing in kaiju_gpu_create ----
  d.sa_full = nullptr; d.text = nullptr; d.row_tax = nullptr; d.tax_of_dense = nullptr; d.n_dense = 0;
  d.row_tax_s = nullptr; d.rts_shift = 0;
  d.beyond_lo = d.beyond_n = d.beyond_row = 0;
  uint64_t text_bytes = 0;
  {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const uint64_t need_peak = pk.bwtlen * 13 + ((uint64_t)pk.nseq << 3) + (64u << 20) + (4ull << 30);   // 9 B per row kept + one temporary of 4 B per row + contexts
    const bool want = !getenv("KAIJU_GPU_NO_TEXT") && !d.mb_base && d.blocks64 && PackedIndex::count(pk.sa_pos, pk.lazy.sa_pos) &&
                      pk.bwtlen + pk.nseq + 4 * (uint64_t)kTextPad < 0xffffffffull && need_peak < free_b / 2;
    if (want) {
      const uint32_t *d_smp = d_stream_sa_pos;
      if (!d_smp && (rc = upload_arr(ix.get(), is, ipath, pk.sa_pos, pk.lazy.sa_pos, &d_smp))) return rc;
      void *smp_alloc = const_cast<uint32_t *>(d_smp);
      uint32_t *row_seq = nullptr, *row_pos = nullptr, *d_len = nullptr, *d_off = nullptr, *d_bad = nullptr, *sa_full = nullptr, *d_beyond = nullptr;
      uint8_t *text = nullptr;
      bool ok = hipMalloc((void **)&row_seq, pk.bwtlen * 4 + 16) == hipSuccess && hipMalloc((void **)&row_pos, pk.bwtlen * 4) == hipSuccess &&
                hipMalloc((void **)&d_len, (size_t)pk.nseq * 4 + 16) == hipSuccess && hipMalloc((void **)&d_off, (size_t)pk.nseq * 4 + 16) == hipSuccess &&
                hipMalloc((void **)&d_bad, 16) == hipSuccess && hipMalloc((void **)&d_beyond, (size_t)kBeyondRowsMax * 4) == hipSuccess;
      if (ok) {
        (void)hipMemset(d_bad, 0, 16);
        (void)hipMemset(d_len, 0, (size_t)pk.nseq * 4);
        const unsigned blocks = (unsigned)std::min<uint64_t>((pk.bwtlen + 255) / 256, 1u << 20);
        hipLaunchKernelGGL(k_suffix_walk, dim3(blocks), dim3(256), 0, 0, d, d_smp, row_seq, row_pos, d_bad, d_beyond);
        hipLaunchKernelGGL(k_seq_lens, dim3((pk.nseq + 255) / 256), dim3(256), 0, 0, pk.nseq, row_seq, row_pos, d_len);
        std::vector<uint32_t> len(pk.nseq), off(pk.nseq);
        uint32_t bad[2] = {0, 0};                           // [1]: rows behind the missing sample of a KAIJU_IDX_WARN_SA_SHORT index
        ok = hipMemcpy(len.data(), d_len, (size_t)pk.nseq * 4, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(bad, d_bad, 8, hipMemcpyDeviceToHost) == hipSuccess && bad[0] == 0 && bad[1] <= kBeyondRowsMax;
        uint64_t at = kTextPad;
        for (uint32_t q = 0; ok && q < pk.nseq; q++) { off[q] = (uint32_t)at; at += (uint64_t)len[q] + 1; if (at + kTextPad >= 0xffffffffull) ok = false; }
        text_bytes = at + 2 * kTextPad;
        ok = ok && hipMemcpy(d_off, off.data(), (size_t)pk.nseq * 4, hipMemcpyHostToDevice) == hipSuccess &&
             hipMalloc((void **)&sa_full, pk.bwtlen * 4 + 64) == hipSuccess && hipMalloc((void **)&text, text_bytes) == hipSuccess;
        if (ok) {
          (void)hipMemset(text, 0, text_bytes);
          hipLaunchKernelGGL(k_text_build, dim3(blocks), dim3(256), 0, 0, d, row_seq, row_pos, d_off, sa_full, text);
          if (bad[1]) hipLaunchKernelGGL(k_rows_beyond, dim3((bad[1] + 255) / 256), dim3(256), 0, 0, d_beyond, bad[1], row_seq);
          ok = hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
          if (ok && bad[1]) {
            // the rows behind the missing sample lie next to each other in the text (one walk: DevIndex::beyond_lo)
            std::vector<uint32_t> rows(bad[1]), tp(bad[1]);
            hipLaunchKernelGGL(k_gather_u32, dim3((bad[1] + 255) / 256), dim3(256), 0, 0, sa_full, d_beyond, bad[1], row_pos);   // (row_pos: free now)
            ok = hipMemcpy(tp.data(), row_pos, (size_t)bad[1] * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                 hipMemcpy(rows.data(), d_beyond, (size_t)bad[1] * 4, hipMemcpyDeviceToHost) == hipSuccess;
            if (ok) {
              const uint32_t lo = *std::min_element(tp.begin(), tp.end()), hi = *std::max_element(tp.begin(), tp.end());
              ok = hi - lo + 1 == bad[1];
              d.beyond_lo = lo; d.beyond_n = bad[1]; d.beyond_row = rows[0];
            }
          }
          if (ok) {
            // row -> sequence -> dense taxon index (the locate's scan over the rows of a match: contiguous loads only)
            std::vector<uint32_t> seq_dense;
            std::vector<uint64_t> tax_of_dense;
            dense_taxa(pk.seq_taxid, pk.seq_valid, seq_dense, tax_of_dense);
            const uint32_t *d_sd = nullptr;
            const uint64_t *d_td = nullptr;
            if (upload(ix.get(), seq_dense, &d_sd) || upload(ix.get(), tax_of_dense, &d_td)) ok = false;
            else {
              hipLaunchKernelGGL(k_row_tax, dim3(blocks), dim3(256), 0, 0, row_seq, pk.bwtlen, d_sd, pk.nseq);
              ok = hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
              ix->allocs.pop_back();                           // (tax_of_dense: re-registered below when everything worked)
              ix->allocs.pop_back();
              (void)hipFree(const_cast<uint32_t *>(d_sd));
              if (ok) { d.tax_of_dense = d_td; d.n_dense = (uint32_t)tax_of_dense.size(); }
              else (void)hipFree(const_cast<uint64_t *>(d_td));
            }
          }
          if (!ok) { d.beyond_lo = d.beyond_n = d.beyond_row = 0; }
        }
      }
      (void)hipGetLastError();
      for (void *q : {(void *)row_pos, (void *)d_len, (void *)d_off, (void *)d_bad, (void *)d_beyond}) if (q) (void)hipFree(q);
      if (!ok && row_seq) { (void)hipFree(row_seq); row_seq = nullptr; }     // (kept otherwise: DevIndex::row_seq)
      // (the sample offsets were only needed here)
      (void)hipFree(smp_alloc);
      ix->allocs.erase(std::find(ix->allocs.begin(), ix->allocs.end(), smp_alloc));
      d_stream_sa_pos = nullptr;
      if (ok) {
        ix->allocs.push_back(sa_full); ix->allocs.push_back(text); ix->allocs.push_back(row_seq);
        ix->allocs.push_back(const_cast<uint64_t *>(d.tax_of_dense));
        d.sa_full = sa_full; d.text = text; d.row_tax = row_seq;
      }
      else { if (sa_full) (void)hipFree(sa_full); if (text) (void)hipFree(text); text_bytes = 0; d.tax_of_dense = nullptr; d.n_dense = 0; }
    }
  }
  if (d_stream_sa_pos) {                                  // (streamed .fmi without text arrays: the sample offsets are not needed)
    (void)hipFree(const_cast<uint32_t *>(d_stream_sa_pos));
    ix->allocs.erase(std::find(ix->allocs.begin(), ix->allocs.end(), (void *)d_stream_sa_pos));
    d_stream_sa_pos = nullptr;
  }
  // ---- the same for an index with 64-bit positions: the text (1 B per row) and the text position of every 2^tv_shift-th row
  //      (5 B each), the densest sample that - with the temporaries of the build and 8 GB for the classification contexts -
  //      fits in 60 % of the free HBM: every row at 4 G rows (26 GB).  Indexes of 2^34 rows and more only on request
  //      (KAIJU_GPU_TV_SHIFT=s forces a sample; every second row at refseq_ref's 28 G rows would be 98 GB next to the index's
  //      92 GB, nothing fits at refseq_nr's 58 G): measured on 4.35 G rows only (profiles/r04_wide_text) ----
  d.sa_tpos5 = nullptr; d.tv_shift = 0;
  uint64_t tpos_bytes = 0, rowtax_bytes = 0;
  // ---- and the row -> taxon table (4 B per row, DevIndex::row_tax): with it the ids of a match are contiguous loads, as on a
  //      narrow index, instead of a walk of up to 2^e LF steps per row - k_mem_locate_wide was the largest kernel of a step
  //      wherever matches hold many rows (a database of protein families at 4.5 G rows: 35 of 47 ms per 2 M reads; refseq_ref's
  //      28 G rows with every protein seven times: 25 of 64 ms).  It comes FIRST when HBM is short (the text arrays save 6 % of
  //      the search kernel, section 5b of DESIGN.md): built when it fits - with 8 GB for the classification contexts - in 70 % of
  //      the free HBM, i.e. up to about 30 G rows on a 288 GB MI355X (112 GB at 28 G rows next to the index's 92 GB);
  //      KAIJU_GPU_ROW_TAX=0 / 1 overrides.  Filled by the same walk of every sequence that writes the text.
  //      An index too big for it (a refseq-class one: 56 - 60 G rows) gets the table of every 2^s-th row, s = 1 .. 3 and below
  //      the exponent of the suffix array's sample (DevIndex::row_tax_s: 60 GB at 60 G rows and s = 2) - the smallest s that
  //      fits by the same rule, or KAIJU_GPU_ROW_TAX_SHIFT=s; the decision is plan_row_tax's (kj_rowtax_plan.h) ----
  // (not on an index with the reference's short sample array: a text-grown match is recorded through the row where the text took
  //  over, the lanes without the arrays record its own end row - and whether that row lies behind the missing sample would then
  //  depend on whether the arrays fit; the narrow lane applies the skip to the grown match itself, DevIndex::beyond_lo.  The
  //  row -> taxon table likewise: the rows behind the missing sample are skipped by the walk, and known only to it)
  if (d.mb_base && d.blocks64 && d.term_pos && !getenv("KAIJU_GPU_NO_TEXT") && pk.bwtlen + 4 * (uint64_t)kTextPad < kTposNone &&
      !(pk.warnings & KAIJU_IDX_WARN_SA_SHORT)) {
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const uint64_t tb_est = pk.bwtlen + 3 * (uint64_t)kTextPad, tmp = (uint64_t)pk.nseq * 20 + 64;
    const RowTaxPlan rtp = plan_row_tax(pk.bwtlen, pk.nseq, pk.chpt_exp, free_b, getenv("KAIJU_GPU_ROW_TAX"), getenv("KAIJU_GPU_ROW_TAX_SHIFT"));
    if (rtp.shift_ignored)
      fprintf(stderr, "[kaiju_gpu load] KAIJU_GPU_ROW_TAX_SHIFT=%s ignored: the shift must be 0 .. %u and below the exponent of the suffix array's sample (%u)\n",
              getenv("KAIJU_GPU_ROW_TAX_SHIFT"), kRowTaxMaxShift, pk.chpt_exp);
    bool rt = rtp.kind != RowTaxPlan::None;
    const uint32_t rt_shift = rtp.shift;
    const double free_tv = (double)free_b - (double)rtp.bytes;      // (the bytes planned: the whole table or the sampled one)
    int tv = -1;
    if (const char *e = getenv("KAIJU_GPU_TV_SHIFT")) { const int v = atoi(e); if (v >= 0 && v <= 8) tv = v; }
    else if (pk.bwtlen < (1ull << 34))
      for (int v = 0; v <= 3 && tv < 0; v++)
        if ((double)(tb_est + ((pk.bwtlen >> v) + 1) * 5 + tmp + (8ull << 30)) <= 0.6 * free_tv) tv = v;
    if (tv >= 0 || rt) {
      uint32_t *t_seq = nullptr, *d_len = nullptr, *d_cnt = nullptr, *row_tax = nullptr;
      uint64_t *d_off = nullptr;
      uint8_t *text = nullptr, *tpos = nullptr;
      const uint32_t *d_sd = nullptr;
      const uint64_t *d_td = nullptr;
      if (tv >= 0) tpos_bytes = ((pk.bwtlen >> tv) + 1) * 5 + 16;
      bool ok = hipMalloc((void **)&t_seq, (size_t)pk.nseq * 4 + 16) == hipSuccess && hipMalloc((void **)&d_len, (size_t)pk.nseq * 4 + 16) == hipSuccess &&
                hipMalloc((void **)&d_off, ((size_t)pk.nseq + 1) * 8) == hipSuccess && hipMalloc((void **)&d_cnt, 16) == hipSuccess;
      if (ok) {
        (void)hipMemset(d_cnt, 0, 16);
        (void)hipMemset(d_len, 0, (size_t)pk.nseq * 4);
        int n_cu = 256;
        { int dev = 0; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev); }
        const unsigned blocks = (unsigned)std::min<uint64_t>(((uint64_t)pk.nseq + 255) / 256, (uint64_t)n_cu * 8);
        hipLaunchKernelGGL(k_seq_walk_len, dim3(blocks), dim3(256), 0, 0, d, d_cnt, t_seq, d_len, d_cnt + 1);
        std::vector<uint32_t> len(pk.nseq);
        std::vector<uint64_t> off((size_t)pk.nseq + 1);
        uint32_t cnt[2] = {0, 0};
        ok = hipMemcpy(len.data(), d_len, (size_t)pk.nseq * 4, hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(cnt, d_cnt, 8, hipMemcpyDeviceToHost) == hipSuccess && cnt[1] == 0;
        off[0] = kTextPad;
        for (uint32_t q = 0; q < pk.nseq; q++) off[(size_t)q + 1] = off[q] + len[q] + 1;
        // (every row lies on exactly one walk: the lengths add up to the rows of the index, or the index is damaged)
        ok = ok && off[pk.nseq] - kTextPad == pk.bwtlen &&
             hipMemcpy(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice) == hipSuccess;
        if (ok && tv >= 0) {
          text_bytes = off[pk.nseq] + 2 * kTextPad;
          // (no room after all, or a text beyond 40-bit positions: the table below is still built)
          if (!(text_bytes < kTposNone && hipMalloc((void **)&text, text_bytes) == hipSuccess && hipMalloc((void **)&tpos, tpos_bytes) == hipSuccess)) {
            (void)hipGetLastError();
            if (text) (void)hipFree(text);
            text = nullptr; tpos = nullptr; text_bytes = 0; tpos_bytes = 0; tv = -1;
          }
        }
        if (ok && rt) {
          std::vector<uint32_t> seq_dense;
          std::vector<uint64_t> tax_of_dense;
          dense_taxa(pk.seq_taxid, pk.seq_valid, seq_dense, tax_of_dense);
          rowtax_bytes = rtp.bytes;                            // (+ slack: the many-rows locate reads 16 bytes at a time)
          if (upload(ix.get(), seq_dense, &d_sd) == 0) { ix->allocs.pop_back(); } else d_sd = nullptr;
          if (d_sd && upload(ix.get(), tax_of_dense, &d_td) == 0) { ix->allocs.pop_back(); } else d_td = nullptr;
          if (!(d_sd && d_td && hipMalloc((void **)&row_tax, rowtax_bytes) == hipSuccess)) {
            (void)hipGetLastError();
            row_tax = nullptr; rowtax_bytes = 0; rt = false;
          } else { d.n_dense = (uint32_t)tax_of_dense.size(); }
        }
        if (ok && (text || row_tax)) {
          if (text) { (void)hipMemset(text, 0, text_bytes); (void)hipMemset(tpos, 0xff, tpos_bytes - 16); (void)hipMemset(tpos + tpos_bytes - 16, 0, 16); }   // (all ones: no entry; the pad is zero)
          if (row_tax) (void)hipMemset(row_tax, 0xff, rowtax_bytes);
          (void)hipMemset(d_cnt, 0, 16);
          hipLaunchKernelGGL(k_seq_walk_fill, dim3(blocks), dim3(256), 0, 0, d, d_cnt, t_seq, d_len, d_off, text, tpos, (uint32_t)std::max(tv, 0), row_tax, d_sd, rt_shift);
          ok = hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
        }
      }
      (void)hipGetLastError();
      for (void *q : {(void *)t_seq, (void *)d_len, (void *)d_off, (void *)d_cnt, (void *)d_sd}) if (q) (void)hipFree(q);
      if (ok && text) { ix->allocs.push_back(text); ix->allocs.push_back(tpos); d.text = text; d.sa_tpos5 = tpos; d.tv_shift = (uint32_t)tv; }
      else { if (text) (void)hipFree(text); if (tpos) (void)hipFree(tpos); text_bytes = 0; tpos_bytes = 0; }
      if (ok && row_tax) {
        ix->allocs.push_back(row_tax); ix->allocs.push_back(const_cast<uint64_t *>(d_td)); d.tax_of_dense = d_td;
        if (rt_shift) { d.row_tax_s = row_tax; d.rts_shift = rt_shift; } else d.row_tax = row_tax;
      }
      else { if (row_tax) (void)hipFree(row_tax); if (d_td) (void)hipFree(const_cast<uint64_t *>(d_td)); rowtax_bytes = 0; d.n_dense = 0; }
    }
    lc.mark("text + text positions, row -> taxon table (device, 64-bit rows)");
  } else
  lc.mark("text + full suffix array (device)");
  kaiju_gpu_index_info &inf = ix->info;
  memset(&inf, 0, sizeof inf);
  inf.bwtlen = (int64_t)pk.bwtlen; inf.nseq = (int32_t)pk.nseq; inf.alen = (int32_t)pk.alen;
  inf.chpt_exp = (int32_t)pk.chpt_exp;
  inf.db_length = (double)((int64_t)pk.bwtlen - (int64_t)pk.nseq);   // Config.cpp:20
  inf.device_bytes = pk.bytes() + kmer_bytes;
  {
    kaiju_gpu_index_footprint &f = ix->fp;
    f.rank_blocks = PackedIndex::count(pk.blocks64, pk.lazy.blocks64) * sizeof(RankBlock64);
    f.count_bases = pk.mb_base.size() * 8;
    f.sa_seq = PackedIndex::count(pk.sa_iseq, pk.lazy.sa_iseq) * 4;
    f.sa_taxid = PackedIndex::count(pk.sa_taxid, pk.lazy.sa_taxid) * 8;
    f.seq_tables = pk.seq_taxid.size() * 8 + pk.seq_valid.size() + PackedIndex::count(pk.term_pos, pk.lazy.term_pos) * 8;
    uint64_t nw = 1;
    for (uint32_t q = 0; q < d.kmer_k; q++) nw *= 20;
    f.kmer_table = d.kmer_k ? nw * (d.kmer64 ? sizeof(ulonglong2) : sizeof(uint2)) : 0;
    uint64_t nlw = 1;
    for (uint32_t q = 1; q < d.kline_k; q++) nlw *= 20;
    f.kmer_lines = d.kline ? nlw * kKLineBytes : 0;
    f.other = sizeof(ConstTables) + sizeof(Stage1Tables) + lnfact.size() * 8 + seg_tab_bytes;
    f.text = d.text ? text_bytes : 0;
    ix->tpos_bytes = d.sa_tpos5 ? tpos_bytes : 0;
    f.sa_full = d.sa_full ? pk.bwtlen * 8 : (d.sa_tpos5 ? tpos_bytes : 0) + (d.mb_base && (d.row_tax || d.row_tax_s) ? rowtax_bytes : 0);   // (+ the taxon of every row, DevIndex::row_tax; wide: the text positions + that table, or the sampled one: row_tax_s)
    f.total = f.rank_blocks + f.count_bases + f.sa_seq + f.sa_taxid + f.seq_tables + f.kmer_table + f.kmer_lines + f.other + f.text + f.sa_full;
    f.kmer_k = std::max(d.kmer_k, d.kline_k); f.wide = d.mb_base ? 1u : 0u;
    inf.device_bytes = f.total;
    if (getenv("KAIJU_GPU_LOAD_TIMES"))
      fprintf(stderr, "[kaiju_gpu load] HBM: rank blocks %.2f GB, count bases %.3f GB, SA sample %.2f (sequence numbers) + %.2f (taxon ids) GB, "
                      "sequence tables %.2f GB, k = %u table %.2f GB + lines %.2f GB, text %.2f GB + full suffix array %.2f GB; %.2f B per index row "
                      "without the k-mer tables\n",
              f.rank_blocks * 1e-9, f.count_bases * 1e-9, f.sa_seq * 1e-9, f.sa_taxid * 1e-9, f.seq_tables * 1e-9, f.kmer_k,
              f.kmer_table * 1e-9, f.kmer_lines * 1e-9, f.text * 1e-9, f.sa_full * 1e-9,
              (double)(f.total - f.kmer_table - f.kmer_lines) / (double)(pk.bwtlen ? pk.bwtlen : 1));
  }
  inf.warnings = pk.warnings;
  snprintf(inf.alphabet, sizeof inf.alphabet, "%s", pk.alphabet.c_str());
  if (keep_packed) ix->names = pk.names; else ix->names.swap(pk.names);    // (keep_packed: further GPUs get the same arrays)
  KJ_HIP(hipDeviceSynchronize());
  *out = ix.release();
  return KAIJU_GPU_OK;
}

// An image of 2 GB and more is streamed to the device (no host copy); a smaller one is read into host memory and uploaded
// from there - allocating the page-locked pieces costs more than streaming saves (viruses-size image, 0.5 GB: 256 against 79 ms,
// profiles/r04_cli).  KAIJU_GPU_IMAGE_HOST_COPY=1: never stream; a piece size in the environment (tests): always.
static bool image_wants_streaming(const char *path) {
  if (getenv("KAIJU_GPU_IMAGE_HOST_COPY")) return false;
  if (getenv("KAIJU_GPU_STREAM_PIECE_KB") || getenv("KAIJU_GPU_STREAM_PIECE_MB")) return true;
  struct stat st;
  return stat(path, &st) == 0 && (uint64_t)st.st_size >= (2ull << 30);
}

// A .fmi of 1 GiB and more goes to the device in pieces and is packed there (fmi_stream.h): no host copy of the file, no packed
// arrays on the host - the loader needs the names of the sequences and two page-locked pieces where PackedIndex::build needs
// twice the file.  KAIJU_GPU_FMI_STREAM=1 / 0: always / never (tests run both ways and compare the device arrays).
static bool fmi_wants_streaming(const char *path) {
  if (const char *e = getenv("KAIJU_GPU_FMI_STREAM")) return atoi(e) != 0;
  struct stat st;
  return stat(path, &st) == 0 && (uint64_t)st.st_size >= (1ull << 30);
}

// does the file start with the magic of an index image?
static bool is_image_file(const char *path) {
  char m[8] = {0};
  FILE *fp = fopen(path, "rb");
  if (!fp) return false;
  const bool ok = fread(m, 1, 8, fp) == 8 && memcmp(m, "KJGPUIM", 7) == 0;
  fclose(fp);
  return ok;
}

extern "C" int kaiju_gpu_index_write_image(const char *fmi_path, const char *image_path) {
  return guarded([&]() -> int {
  if (!fmi_path || !image_path) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  std::unique_ptr<FmiFile> f(new FmiFile());
  std::string msg;
  LoadClock lc;
  int rc = f->load(fmi_path, msg);
  lc.mark("read .fmi file");
  if (rc) return fail(rc, msg);
  PackedIndex pk;
  if ((rc = pk.build(f->view(), msg))) return fail(rc, msg);
  f.reset();                        // (a refseq-class .fmi is 60 GB in memory: gone before the image, as large again, is written)
  lc.mark("pack (host)");
  { struct stat st; if (stat(fmi_path, &st) == 0) pk.src_fmi_bytes = (uint64_t)st.st_size; }
  if ((rc = pk.write_image(image_path, msg))) return fail(rc, msg);
  lc.mark("write image file");
  return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_index_image_source_bytes(const char *image_path, uint64_t *fmi_bytes) {
  return guarded([&]() -> int {
  if (!image_path || !fmi_bytes) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  std::string msg;
  const int rc = PackedIndex::image_source_bytes(image_path, *fmi_bytes, msg);
  return rc ? fail(rc, msg) : KAIJU_GPU_OK;
  });
}

// Host only: what an image file holds, read the way the loader reads it (header and the small arrays; the arrays that grow with
// the index are only located) - a caller can check an image and see how many bytes a load streams to the device without a GPU.
extern "C" int kaiju_gpu_index_image_info(const char *image_path, kaiju_gpu_index_info *info, uint64_t *streamed_bytes) {
  return guarded([&]() -> int {
  if (!image_path || !info) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (!is_image_file(image_path)) return fail(KAIJU_GPU_ERR_FORMAT, "not a kaiju GPU index image");
  PackedIndex pk;
  std::string msg;
  const int rc = pk.read_image(image_path, msg, true);
  if (rc) return fail(rc, msg);
  memset(info, 0, sizeof *info);
  info->bwtlen = (int64_t)pk.bwtlen; info->nseq = (int32_t)pk.nseq; info->alen = (int32_t)pk.alen; info->chpt_exp = (int32_t)pk.chpt_exp;
  info->db_length = (double)((int64_t)pk.bwtlen - (int64_t)pk.nseq);
  info->device_bytes = pk.bytes();
  info->warnings = pk.warnings;
  snprintf(info->alphabet, sizeof info->alphabet, "%s", pk.alphabet.c_str());
  if (streamed_bytes) {
    const ImageLazy &l = pk.lazy;
    *streamed_bytes = l.blocks64.n * sizeof(RankBlock64) + l.sa_iseq.n * 4 + l.sa_pos.n * 4 + l.term_pos.n * 8 + l.kmer32.n * sizeof(uint2) +
                      l.kmer64.n * sizeof(ulonglong2);
  }
  return KAIJU_GPU_OK;
  });
}

extern "C" int kaiju_gpu_index_load(const char *fmi_path, int device_id, kaiju_gpu_index **out) {
  return guarded([&]() -> int {
  if (!fmi_path || !out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  *out = nullptr;
  std::future<int> dev = device_check_async(device_id);
  if (is_image_file(fmi_path)) {
    // a pre-packed image (kaiju_gpu_index_write_image): no parsing, no packing
    PackedIndex pk;
    std::string msg;
    LoadClock lc;
    // the arrays that grow with the index are streamed from the file to the device (kaijux ids rewrite the sampled ids on the
    // host: that mode reads everything; KAIJU_GPU_IMAGE_HOST_COPY=1 does so too, for comparison)
    const bool lazy = tl_id_mode == 0 && image_wants_streaming(fmi_path);
    const int rc = pk.read_image(fmi_path, msg, lazy);
    lc.mark(lazy ? "read image file (small arrays)" : "read image file");
    const int drc = device_check_result(dev);
    lc.mark("wait for the HIP runtime");
    if (drc) return drc;
    if (rc) return fail(rc, msg);
    return index_from_packed(pk, device_id, out);
  }
  FmiFile f;
  std::string msg;
  LoadClock lc;
  const bool streamed = fmi_wants_streaming(fmi_path);
  int rc = f.load(fmi_path, msg, streamed);
  lc.mark(streamed ? "read .fmi file (headers, names)" : "read .fmi file");
  if (rc) { const int drc = device_check_result(dev); return drc ? drc : fail(rc, msg); }
  if (!streamed) return index_from_view(f.view(), device_id, out, &dev);
  // the BWT and the sampled suffix array stay in the file: they are streamed to the device and packed there (fmi_stream.h)
  PackedIndex pk;
  rc = pk.build_streamed(f, fmi_path, msg);
  { std::vector<std::string>().swap(f.ids); std::vector<const char *>().swap(f.id_ptrs); }    // (pk has its own copy of the names)
  lc.mark("names, taxon ids (host)");
  const int drc = device_check_result(dev);
  lc.mark("wait for the HIP runtime");
  if (drc) return drc;
  if (rc) return fail(rc, msg);
  return index_from_packed(pk, device_id, out);
  });
}

extern "C" int kaiju_gpu_index_load_ex(const char *fmi_path, int device_id, int id_mode, kaiju_gpu_index **out) {
  if (id_mode != KAIJU_GPU_IDS_TAXON && id_mode != KAIJU_GPU_IDS_SEQUENCE) return fail(KAIJU_GPU_ERR_ARG, "id_mode");
  tl_id_mode = id_mode;
  const int rc = kaiju_gpu_index_load(fmi_path, device_id, out);
  tl_id_mode = 0;
  return rc;
}

// One index, several GPUs of a node: the file is parsed and packed (or its image read) ONCE, the packed arrays go to every
// device in turn; each device grows its own k-mer table, lines and text arrays.  out[k] belongs to devices[k].
extern "C" int kaiju_gpu_index_load_devices(const char *fmi_path, const int *devices, int n_devices, int id_mode, kaiju_gpu_index **out) {
  return guarded([&]() -> int {
  if (!fmi_path || !devices || !out || n_devices < 1) return fail(KAIJU_GPU_ERR_ARG, "bad argument");
  if (id_mode != KAIJU_GPU_IDS_TAXON && id_mode != KAIJU_GPU_IDS_SEQUENCE) return fail(KAIJU_GPU_ERR_ARG, "id_mode");
  for (int k = 0; k < n_devices; k++) out[k] = nullptr;
  std::future<int> dev = device_check_async(devices[0]);
  PackedIndex pk;
  std::string msg;
  int rc;
  if (is_image_file(fmi_path)) rc = pk.read_image(fmi_path, msg, id_mode == 0 && image_wants_streaming(fmi_path));
  else {
    FmiFile f;
    const bool streamed = fmi_wants_streaming(fmi_path);      // (every device then streams the file for itself: it is in the page cache)
    rc = f.load(fmi_path, msg, streamed);
    if (rc == 0) rc = streamed ? pk.build_streamed(f, fmi_path, msg) : pk.build(f.view(), msg);
  }
  const int drc = device_check_result(dev);
  if (drc) return drc;
  if (rc) return fail(rc, msg);
  tl_id_mode = id_mode;
  for (int k = 0; k < n_devices && rc == 0; k++) rc = index_from_packed(pk, devices[k], &out[k], k + 1 < n_devices);
  tl_id_mode = 0;
  if (rc) for (int k = 0; k < n_devices; k++) { delete out[k]; out[k] = nullptr; }
  return rc;
  });
}

extern "C" int kaiju_gpu_index_from_host(const kaiju_gpu_host_index *hv, int device_id, kaiju_gpu_index **out) {
  return guarded([&]() -> int {
  if (!hv || !out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  HostIndexView v;
  v.bwtlen = hv->bwtlen; v.nseq = hv->nseq; v.alen = hv->alen; v.alphabet = hv->alphabet; v.bwt = hv->bwt;
  v.startLcode = hv->startLcode; v.sa = hv->sa; v.ncheck = hv->ncheck; v.chpt_exp = hv->chpt_exp;
  v.nbytes = hv->nbytes; v.pbits = hv->pbits; v.ids = hv->ids;
  return index_from_view(v, device_id, out);
  });
}

extern "C" int kaiju_gpu_index_get_info(const kaiju_gpu_index *ix, kaiju_gpu_index_info *info) {
  if (!ix || !info) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  *info = ix->info;
  return KAIJU_GPU_OK;
}
extern "C" int kaiju_gpu_index_get_footprint(const kaiju_gpu_index *ix, kaiju_gpu_index_footprint *out) {
  if (!ix || !out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  *out = ix->fp;
  return KAIJU_GPU_OK;
}
extern "C" void kaiju_gpu_index_free(kaiju_gpu_index *ix) { delete ix; }

// digest of `n` bytes: the sum over all 16-byte chunks of a mix of (chunk number, content); the last chunk is zero-padded
__global__ void __launch_bounds__(256)
k_digest(const uint8_t *__restrict__ p, uint64_t n, unsigned long long *out) {
  const uint64_t chunks = (n + 15) >> 4;
  uint64_t acc = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * 256) {
    uint32_t w[4] = {0, 0, 0, 0};
    if ((c << 4) + 16 <= n && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
      const uint4 v = reinterpret_cast<const uint4 *>(p)[c];
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
      for (uint32_t b = 0; b < 16 && (c << 4) + b < n; b++) w[b >> 2] |= (uint32_t)p[(c << 4) + b] << (8 * (b & 3));
    }
    uint64_t h = (c + 1) * 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int q = 0; q < 4; q++) { h ^= w[q]; h *= 0xD6E8FEB86659FD93ull; h ^= h >> 29; }
    acc += h;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if ((threadIdx.x & 63u) == 0) atomicAdd(out, (unsigned long long)acc);
}

extern "C" int kaiju_gpu_index_digest(const kaiju_gpu_index *ix, uint64_t *out, uint32_t n_out) {
  return guarded([&]() -> int {
  if (!ix || !out || n_out < KAIJU_GPU_N_DIGESTS) return fail(KAIJU_GPU_ERR_ARG, "bad argument");
  KJ_HIP(hipSetDevice(ix->device));
  const DevIndex &d = ix->dev;
  IndexArr arrs[kIndexArrays];                     // (the digest covers the first twelve: tax_of_dense came later, out[] is ABI)
  index_arrays(d, ix->fp.text, ix->tpos_bytes, arrs);
  unsigned long long *acc = nullptr;
  KJ_HIP(hipMalloc((void **)&acc, 12 * 8));
  hipError_t e = hipMemset(acc, 0, 12 * 8);
  for (int a = 0; a < 12 && e == hipSuccess; a++) {
    if (!arrs[a].p || !arrs[a].bytes) continue;
    const uint64_t chunks = (arrs[a].bytes + 15) >> 4;
    hipLaunchKernelGGL(k_digest, dim3((unsigned)std::min<uint64_t>((chunks + 255) / 256, 1u << 16)), dim3(256), 0, 0,
                       static_cast<const uint8_t *>(arrs[a].p), arrs[a].bytes, acc + a);
    e = hipGetLastError();
  }
  unsigned long long h[12] = {0};
  if (e == hipSuccess) e = hipMemcpy(h, acc, sizeof h, hipMemcpyDeviceToHost);
  (void)hipFree(acc);
  if (e != hipSuccess) return fail(KAIJU_GPU_ERR_HIP, hipGetErrorString(e));
  for (int a = 0; a < 12; a++) out[a] = h[a];
  out[12] = d.kmer_k | (uint64_t)d.kline_k << 8;
  uint64_t hc = 0;
  for (int a = 0; a < 22; a++) hc = (hc ^ d.C[a]) * 0xD6E8FEB86659FD93ull + 1;
  out[13] = hc;
  return KAIJU_GPU_OK;
  });
}

// Diagnostics: the arrays of an index as they lie in HBM (include/kaiju_gpu.h) - sizes and scalars, and a plain copy of a slice
static_assert(kIndexArrays == KAIJU_GPU_N_INDEX_ARRAYS, "kj::index_arrays and the header list the same arrays");
extern "C" int kaiju_gpu_index_get_layout(const kaiju_gpu_index *ix, kaiju_gpu_index_layout *out) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (!ix || !out) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  const DevIndex &d = ix->dev;
  IndexArr arrs[kIndexArrays];
  index_arrays(d, ix->fp.text, ix->tpos_bytes, arrs);
  memset(out, 0, sizeof *out);
  for (int a = 0; a < kIndexArrays; a++) out->bytes[a] = arrs[a].bytes;
  for (int a = 0; a < 22; a++) out->C[a] = d.C[a];
  out->bwtlen = d.bwtlen; out->n_sa = d.n_sa; out->sa_skip = d.sa_skip; out->nseq = d.nseq; out->chpt_exp = d.chpt_exp;
  out->mb_shift = d.mb_shift; out->kmer_k = d.kmer_k; out->kline_k = d.kline_k; out->tv_shift = d.tv_shift; out->n_dense = d.n_dense;
  out->beyond_lo = d.beyond_lo; out->beyond_n = d.beyond_n; out->beyond_row = d.beyond_row; out->wide = d.mb_base ? 1u : 0u;
  out->row_tax_shift = d.row_tax_s ? d.rts_shift : 0u;
  return KAIJU_GPU_OK;
  });
}
extern "C" int kaiju_gpu_index_read_array(const kaiju_gpu_index *ix, uint32_t which, uint64_t offset_bytes, uint64_t n_bytes, void *host_out) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (!ix || (!host_out && n_bytes) || which >= (uint32_t)kIndexArrays) return fail(KAIJU_GPU_ERR_ARG, "bad argument");
  IndexArr arrs[kIndexArrays];
  index_arrays(ix->dev, ix->fp.text, ix->tpos_bytes, arrs);
  const IndexArr &a = arrs[which];
  if (offset_bytes > a.bytes || n_bytes > a.bytes - offset_bytes) return fail(KAIJU_GPU_ERR_ARG, "slice beyond the array");
  if (n_bytes == 0) return KAIJU_GPU_OK;
  KJ_HIP(hipSetDevice(ix->device));
  KJ_HIP(hipMemcpy(host_out, static_cast<const uint8_t *>(a.p) + offset_bytes, n_bytes, hipMemcpyDeviceToHost));
  return KAIJU_GPU_OK;
  });
}

// ---- the name tables of the index: accessions (kaiju -v) and sequence names (kaijux / kaijup) ----
// K host arrays to device memory of the index (16 bytes of slack each): all of them or none; the pointers join ix->allocs
template <int K>
static int upload_table(kaiju_gpu_index *ix, const void *const (&src)[K], const size_t (&bytes)[K], void *(&d)[K], const char *what) {
  KJ_HIP(hipSetDevice(ix->device));
  for (int k = 0; k < K; k++) d[k] = nullptr;
  for (int k = 0; k < K; k++) {
    if (hipMalloc(&d[k], bytes[k] + 16) != hipSuccess || hipMemcpy(d[k], src[k], bytes[k], hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      for (int j = 0; j <= k; j++) if (d[j]) (void)hipFree(d[j]);
      return fail(KAIJU_GPU_ERR_NOMEM, what);
    }
  }
  for (int k = 0; k < K; k++) ix->allocs.push_back(d[k]);
  return KAIJU_GPU_OK;
}

static std::mutex g_acc_mutex;      // the accession tables of all indexes: upload against upload, upload against the readers below
extern "C" int kaiju_gpu_index_upload_accessions(kaiju_gpu_index *ix) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format_verbose()) return rc;
  if (!ix) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  if (ix->id_mode != KAIJU_GPU_IDS_TAXON) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "an index of sequence ids (kaijux / kaijup) has no accession column");
  std::lock_guard<std::mutex> lk(g_acc_mutex);
  if (ix->acc_ready) return KAIJU_GPU_OK;
  const size_t nseq = ix->names.size();
  if (nseq >= 0xffffffffull) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "more than 2^32 - 2 sequences");
  std::vector<const char *> ptr(nseq);
  for (size_t i = 0; i < nseq; i++) ptr[i] = ix->names[i].c_str();
  std::vector<uint32_t> rank(nseq + 1), len(nseq + 1);
  if (int rc = kaiju_accession_ranks(ptr.data(), (uint32_t)nseq, rank.data(), len.data())) return fail(rc, "kaiju_accession_ranks");
  std::vector<uint64_t> aoff(nseq + 1);
  uint64_t total = 0;
  for (size_t i = 0; i < nseq; i++) {
    if (len[i] > kjv::kMaxPrefix) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "a sequence name of the index is longer than 2^24 bytes");
    aoff[i] = total; total += len[i];
  }
  aoff[nseq] = total;
  std::vector<uint8_t> blob((size_t)total + 1);
  for (size_t i = 0; i < nseq; i++) if (len[i]) memcpy(blob.data() + aoff[i], ptr[i], len[i]);
  void *d[4];
  if (int rc = upload_table<4>(ix, {blob.data(), aoff.data(), len.data(), rank.data()}, {(size_t)total + 1, (nseq + 1) * 8, (nseq + 1) * 4, (nseq + 1) * 4},
                               d, "the accession table could not be uploaded")) return rc;
  ix->acc_blob = static_cast<const uint8_t *>(d[0]); ix->acc_off = static_cast<const uint64_t *>(d[1]);
  ix->acc_len = static_cast<const uint32_t *>(d[2]); ix->acc_rank = static_cast<const uint32_t *>(d[3]);
  ix->acc_bytes = total + 16 * (uint64_t)nseq;
  ix->acc_ready = true;
  return KAIJU_GPU_OK;
  });
}
extern "C" uint64_t kaiju_gpu_index_accession_bytes(const kaiju_gpu_index *ix) {
  if (!ix) return 0;
  std::lock_guard<std::mutex> lk(g_acc_mutex);
  return ix->acc_ready ? ix->acc_bytes : 0;
}
bool index_accessions(const kaiju_gpu_index *ix, kjv::Job &J) {
  std::lock_guard<std::mutex> lk(g_acc_mutex);
  if (!ix->acc_ready) return false;
  J.acc_blob = ix->acc_blob; J.acc_off = ix->acc_off; J.acc_len = ix->acc_len; J.acc_rank = ix->acc_rank;
  return true;
}

static std::mutex g_sn_mutex;       // the sequence-name tables of all indexes: upload against upload, upload against the readers below
extern "C" int kaiju_gpu_index_upload_seq_names(kaiju_gpu_index *ix) {
  return guarded([&]() -> int {
  if (int rc = no_device()) return rc;
  if (int rc = no_format_seq()) return rc;
  if (!ix) return fail(KAIJU_GPU_ERR_ARG, "NULL argument");
  std::lock_guard<std::mutex> lk(g_sn_mutex);
  if (ix->sn_ready) return KAIJU_GPU_OK;
  const size_t nseq = ix->names.size();
  if (nseq >= 0xffffffffull) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "more than 2^32 - 2 sequences");
  std::vector<uint64_t> noff(nseq + 1);
  std::vector<uint32_t> len(nseq + 1);
  uint64_t total = 0;
  uint32_t longest = 0;
  for (size_t i = 0; i < nseq; i++) {
    // (what kaiju_gpu_index_seq_name hands out: the name as a C string)
    const size_t l = strlen(ix->names[i].c_str());
    if (l > kjq::kMaxSeqName) return fail(KAIJU_GPU_ERR_UNSUPPORTED, "a sequence name of the index is longer than 2^24 bytes");
    len[i] = (uint32_t)l; noff[i] = total; total += l;
    longest = std::max(longest, len[i]);
  }
  noff[nseq] = total;
  std::vector<uint8_t> blob((size_t)total + 1);
  for (size_t i = 0; i < nseq; i++) if (len[i]) memcpy(blob.data() + noff[i], ix->names[i].c_str(), len[i]);
  void *d[3];
  if (int rc = upload_table<3>(ix, {blob.data(), noff.data(), len.data()}, {(size_t)total + 1, (nseq + 1) * 8, (nseq + 1) * 4}, d,
                               "the sequence-name table could not be uploaded")) return rc;
  ix->sn_blob = static_cast<const uint8_t *>(d[0]); ix->sn_off = static_cast<const uint64_t *>(d[1]); ix->sn_len = static_cast<const uint32_t *>(d[2]);
  ix->sn_bytes = total + 12 * (uint64_t)nseq;
  ix->sn_max = longest;
  ix->sn_ready = true;
  return KAIJU_GPU_OK;
  });
}
extern "C" uint64_t kaiju_gpu_index_seq_name_bytes(const kaiju_gpu_index *ix) {
  if (!ix) return 0;
  std::lock_guard<std::mutex> lk(g_sn_mutex);
  return ix->sn_ready ? ix->sn_bytes : 0;
}
bool index_seq_names(const kaiju_gpu_index *ix, kjq::Job &J) {
  std::lock_guard<std::mutex> lk(g_sn_mutex);
  if (!ix->sn_ready) return false;
  J.sn_blob = ix->sn_blob; J.sn_off = ix->sn_off; J.sn_len = ix->sn_len;
  return true;
}
