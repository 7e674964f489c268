// fq_frontend.cpp -- host side of the FASTQ front end on the device (kernels: fq_frontend.h).
//
// Replaces, for BGZF files of four-line records, the reader side of bwa_read_seq_with_hash_dev (src/BwtMapper.cpp:476-613): gzread
// (libbwa/bwaseqio.c:41-52) under kseq_read3_fpc (libbwa/kseq.h:327-371) on one IO thread per file (IOworkerAlt, src/BwtMapper.cpp:1973-1980).
// The host reads compressed bytes and walks the members' headers (18 bytes per 64 KiB of text); everything per byte of text happens in HBM.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/fastquick_amd.h"
#include "fq_backend.h"
#include "fq_inflate.h"

namespace {
// ---- BGZF members of a compressed image (SAM spec 4.1: gzip members with a 'BC' extra subfield that states the member's size) ----
struct HostMember { size_t at, size, hdr; uint32_t isize, crc; };
// size of the member that starts at h (>= 18 readable bytes), 0 if it is not a BGZF member
size_t bgzf_member(const uint8_t *h, size_t n, size_t *hdr_len) {
  if (n < 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return 0;
  const size_t xlen = h[10] | (size_t)h[11] << 8;
  if (12 + xlen > n) return 0;
  size_t p = 12;
  while (p + 4 <= 12 + xlen) {
    const size_t sl = h[p + 2] | (size_t)h[p + 3] << 8;
    if (h[p] == 'B' && h[p + 1] == 'C' && sl == 2 && p + 6 <= 12 + xlen) { *hdr_len = 12 + xlen; return (size_t)(h[p + 4] | (size_t)h[p + 5] << 8) + 1; }
    p += 4 + sl;
  }
  return 0;
}
inline uint32_t le32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
// the whole members of [p, p + n): false when something that is not a member stands at a member boundary
bool walk_members(const uint8_t *p, size_t n, std::vector<HostMember> &ms, size_t *consumed) {
  size_t at = 0;
  while (n - at >= 18) {
    size_t hdr = 0;
    const size_t sz = bgzf_member(p + at, n - at, &hdr);
    if (sz == 0) { *consumed = at; return false; }
    if (sz < hdr + 8) { *consumed = at; return false; }
    if (n - at < sz) break;
    ms.push_back({at, sz, hdr, le32(p + at + sz - 4), le32(p + at + sz - 8)});
    at += sz;
  }
  *consumed = at;
  return true;
}

struct DevScope {
  fqdev::State *s;
  explicit DevScope(int dev) : s(fqdev::state_create(dev)) {}
  ~DevScope() { fqdev::state_destroy(s); }
};
struct DevMem {
  void *p = nullptr;
  ~DevMem() { fqdev::dfree(p); }
  bool alloc(size_t n) { p = fqdev::dmalloc(n); return p != nullptr; }
};
}  // namespace

// ---- the member decoder on its own (tests, measurement) ----------------------------------------------------------------------------
// n_streams raw DEFLATE streams (RFC 1951) src[k] of n[k] bytes, each promising out_len[k] bytes with CRC-32 crc[k], inflated by the
// device's decoder -- one wavefront per stream -- into dst[k] (out_len[k] bytes each); status[k] = 0 inflated and checked, 1 refused
// (a stream the device does not take: the reader hands such a member to fq_inflate.h, then zlib), 2 CRC mismatch.
extern "C" int fq_inflate_device(int device, int n_streams, const uint8_t *const *src, const size_t *n, uint8_t *const *dst, const uint32_t *out_len, const uint32_t *crc,
                                 uint32_t *status, int repeats, double *kernel_ms) {
  if (n_streams < 0 || (n_streams && (!src || !n || !dst || !out_len || !crc || !status))) return FQ_EINVAL;
  DevScope scope(device);
  if (!scope.s || fqdev::bind(scope.s)) return FQ_ENODEV;
  std::vector<FqzMember> mem((size_t)n_streams);
  size_t c_total = 0, o_total = 0;
  for (int k = 0; k < n_streams; ++k) {
    if (n[k] > 0xffffffffull) return FQ_ELIMIT;
    if (o_total + out_len[k] > 0xfffffff0ull) return FQ_ELIMIT;      // (32-bit text positions inside one launch)
    mem[k].in_off = c_total; mem[k].in_len = (uint32_t)n[k]; mem[k].out_off = (uint32_t)o_total; mem[k].out_len = out_len[k]; mem[k].crc = crc[k]; mem[k].pad[0] = mem[k].pad[1] = 0;
    c_total += n[k] + (k % 3);       // (members of a file follow each other at any alignment)
    o_total += out_len[k];
  }
  std::vector<uint8_t> comp(c_total + 1024 + 16, 0);
  for (int k = 0; k < n_streams; ++k) if (n[k]) memcpy(comp.data() + mem[k].in_off, src[k], n[k]);
  DevMem d_comp, d_out, d_mem, d_status;
  if (!d_comp.alloc(comp.size()) || !d_out.alloc(o_total + 512) || !d_mem.alloc(sizeof(FqzMember) * (size_t)std::max(1, n_streams)) || !d_status.alloc(4 * (size_t)std::max(1, n_streams))) return FQ_ENOMEM;
  const FqzCrcConst *cc = fqdev::crc_const();
  if (!cc) return FQ_ENODEV;
  if (fqdev::h2d(d_comp.p, comp.data(), comp.size()) || fqdev::h2d(d_mem.p, mem.data(), sizeof(FqzMember) * mem.size()) || fqdev::dzero(d_out.p, o_total + 512) || fqdev::sync()) return FQ_ENODEV;
  FqInflateArgs a{};
  a.comp = (const uint8_t *)d_comp.p; a.mem = (const FqzMember *)d_mem.p; a.n_mem = n_streams; a.out = (uint8_t *)d_out.p; a.status = (uint32_t *)d_status.p; a.crc = cc;
  double ms[FQ_K_COUNT] = {0};
  uint64_t launches[FQ_K_COUNT] = {0};
  for (int r = 0; r < std::max(1, repeats); ++r) {
    fqdev::time_begin(0);
    if (fqdev::launch_inflate(a)) return FQ_ENODEV;
    fqdev::time_end(0);
  }
  if (fqdev::sync()) return FQ_ENODEV;
  fqdev::time_collect(ms, launches, FQ_K_COUNT);
  if (kernel_ms) *kernel_ms = launches[0] ? ms[0] / (double)launches[0] : 0.0;
  std::vector<uint8_t> out(o_total + 1);
  if (fqdev::d2h(out.data(), d_out.p, o_total) || fqdev::d2h(status, d_status.p, 4 * (size_t)n_streams) || fqdev::sync()) return FQ_ENODEV;
  for (int k = 0; k < n_streams; ++k) if (out_len[k]) memcpy(dst[k], out.data() + mem[k].out_off, out_len[k]);
  return FQ_OK;
}

// The members of a BGZF image (a whole file, or any run of whole members) inflated on the device into `out` (their text back to back).
// status[k] per member as above (NULL: not wanted); *n_members, *text_len: what was found.  FQ_EIO: not a run of BGZF members;
// FQ_ELIMIT: out_cap too small.
extern "C" int fq_bgzf_inflate_device(int device, const uint8_t *file, size_t n, uint8_t *out, size_t out_cap, int64_t *n_members, int64_t *text_len, uint32_t *status, int64_t status_cap,
                                      int repeats, double *kernel_ms) {
  if (!file || !out) return FQ_EINVAL;
  std::vector<HostMember> ms;
  size_t used = 0;
  if (!walk_members(file, n, ms, &used) || used != n) return FQ_EIO;
  std::vector<const uint8_t *> src;
  std::vector<size_t> len;
  std::vector<uint8_t *> dst;
  std::vector<uint32_t> olen, crc;
  size_t o = 0;
  for (const auto &m : ms) {
    if (m.isize == 0) continue;          // (the empty end-of-file member)
    src.push_back(file + m.at + m.hdr); len.push_back(m.size - m.hdr - 8); dst.push_back(out + o); olen.push_back(m.isize); crc.push_back(m.crc);
    o += m.isize;
    if (o > out_cap) return FQ_ELIMIT;
  }
  if (n_members) *n_members = (int64_t)src.size();
  if (text_len) *text_len = (int64_t)o;
  std::vector<uint32_t> st(src.size() + 1);
  const int rc = fq_inflate_device(device, (int)src.size(), src.data(), len.data(), dst.data(), olen.data(), crc.data(), st.data(), repeats, kernel_ms);
  if (rc) return rc;
  if (status) memcpy(status, st.data(), 4 * (size_t)std::min<int64_t>(status_cap, (int64_t)src.size()));
  return FQ_OK;
}

// =====================================================================================================================================
// The reader: one FASTQ pair (or one single-end file) -> batches whose text, records, filter keys and names are resident in HBM.
//
//   reader threads (one per file)   pread the compressed bytes of the next chunk into pinned staging, walk the members' headers, upload
//   the producer thread             inflates the chunk's members (k_inflate_bgzf; a member the device refuses: fq_inflate.h, then zlib),
//                                   indexes the line ends, checks and cuts the records, forms the filter's keys, walks the read slots,
//                                   writes the names -- and queues the batch
//   fq_frontend_next()              hands the next batch to the caller (who gives it to fq_align_text)
//
// A chunk holds whole reference batches (batch_pairs: insert sizes are inferred per reference batch, libbwa/bwape.c:49-117) unless it is
// the stream's last.  Text behind a chunk's last record stays in HBM and leads the next chunk.  Whatever the device does not take -- a
// record that is not four plain lines, a file that ends inside a record, a member neither decoder accepts -- ends the device's part of the
// stream at a reference-batch boundary: fq_frontend_next() returns FQ_EFALLBACK and fq_frontend_handover() gives the host readers
// (fq_fastq.cpp) standing exactly there, read slots included; their verdicts stand.
// =====================================================================================================================================
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <zlib.h>

#include "fq_fastq_internal.h"

#include "fq_text_batch.h"

namespace {
template <class T> struct DBuf {
  T *p = nullptr; size_t cap = 0;
  ~DBuf() { fqdev::dfree(p); }
  bool ensure(size_t n) {
    if (n <= cap) return true;
    fqdev::dfree(p);
    cap = n + n / 8 + 256;
    p = (T *)fqdev::dmalloc(cap * sizeof(T));
    if (!p) cap = 0;
    return p != nullptr;
  }
  bool ensure_keep(size_t n, size_t keep) {   // the first `keep` elements survive (copied on the bound state's stream, then waited for)
    if (n <= cap) return true;
    const size_t ncap = n + n / 8 + 256;
    T *q = (T *)fqdev::dmalloc(ncap * sizeof(T));
    if (!q) return false;
    if (keep && (fqdev::d2d(q, p, keep * sizeof(T)) || fqdev::sync())) { fqdev::dfree(q); return false; }
    fqdev::dfree(p); p = q; cap = ncap;
    return true;
  }
};
template <class T> struct HBuf {
  T *p = nullptr; size_t cap = 0;
  ~HBuf() { fqdev::hfree(p); }
  bool ensure(size_t n) {
    if (n <= cap) return true;
    fqdev::hfree(p);
    cap = n + n / 8 + 256;
    p = (T *)fqdev::hmalloc(cap * sizeof(T));
    if (!p) cap = 0;
    return p != nullptr;
  }
};
const size_t kPiece = (size_t)32 << 20;       // pinned staging pieces of the compressed stream
const uint64_t kMaxText = (uint64_t)3500 << 20;   // text positions are 32-bit inside a launch
const int kSlots = 4;                          // batches: two with the caller (one under its kernels, one under its consumers), one being tokenised, one being inflated

struct CompChunk {                             // one file's compressed bytes of one chunk, in HBM, with their member table
  DBuf<uint8_t> d_comp;
  DBuf<FqzMember> d_mem;
  DBuf<uint32_t> d_status;
  std::vector<FqzMember> mem;                  // out_off relative to the chunk's first new byte of text
  size_t comp_len = 0;
  uint64_t text_len = 0;
  int64_t file_off_end = 0;                    // file offset behind the chunk's last member
  bool eof = false;
  std::string err;
};
struct FileSide {
  std::string path;
  int fd = -1;
  int64_t file_off = 0;                        // next byte to read
  bool file_eof = false;
  std::vector<uint8_t> tail;                   // bytes of an incomplete member at the end of what was read
  fqdev::State *st = nullptr;                  // the reader thread's device state (its stream carries the uploads)
  HBuf<uint8_t> pin[2];
  CompChunk chunk[3];                          // the reader runs up to two chunks ahead of the inflation
  std::thread th;
  // hand-shake with the producer: chunk slots are filled by the reader in turn and released by the producer in the same order
  std::mutex mu;
  std::condition_variable cv;
  bool filled[3] = {false, false, false};
  uint64_t want_text = 0;                      // text a chunk should hold (the producer's latest estimate)
  double want_scale = 1.0;                     // BAM input: payload bytes of the one compressed side per byte of the first side's text
  bool stop = false;
  int64_t inflated_file_off = 0;               // the file offset behind the last chunk that has been inflated
  // text
  DBuf<uint8_t> d_text[kSlots];                // one per batch slot
  DBuf<uint32_t> d_nl;
  uint64_t carry_off = 0, carry_len = 0;       // the text behind the last chunk's records: in d_text[carry_slot]
  int carry_slot = -1;
  int64_t records_done = 0;                    // records of this file in batches so far
  double text_per_record = 0;
  bool all_launched = false;                   // every member of the file has been handed to the decoder
  // slots
  DBuf<uint8_t> d_slot_base, d_slot_name;
  DBuf<uint16_t> d_slot_len;
  DBuf<uint32_t> d_stat;
  int shorter_after_longer = 0;
  uint64_t file_size = 0;
  double comp_ratio = 0.4;                     // compressed bytes per byte of text (the first member's; then the last chunk's)
  int chunks_read = 0;                         // (by the reader thread)
  int read_threads = 1;                        // threads of one pread_threads call
  double ms_read = 0, ms_upload = 0;           // the reader thread's time in pread / in uploads (fq_frontend_stats)
};
inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
}  // namespace

namespace {
// ---- BAM input (fq_bamin.h): the scratch of the transcoding kernels, and what a stream keeps from chunk to chunk ----
// the wanted IDs as fq_bamin.h's tag body reads them, on the device and in the probe: dwords -- their count, their lengths, then their bytes
void pack_bam_ids(const fq_bam_select_t *sl, std::vector<uint32_t> *out) {
  out->clear();
  const int32_t n = sl && sl->ids ? std::max<int32_t>(sl->n_ids, 0) : 0;
  if (!n) return;
  std::string bytes;
  out->push_back((uint32_t)n);
  for (int32_t k = 0; k < n; ++k) { const std::string id = sl->ids[k] ? sl->ids[k] : ""; out->push_back((uint32_t)id.size()); bytes += id; }
  bytes.resize((bytes.size() + 4) & ~(size_t)3);
  const size_t at = out->size();
  out->resize(at + bytes.size() / 4);
  memcpy(out->data() + at, bytes.data(), bytes.size());
}
struct BamWork {
  DBuf<uint32_t> seg, res, starts, kept, kidx, len[2], src[2];
  DBuf<uint64_t> base, kord, off[2], bad;
  std::vector<uint32_t> h_seg, h_res;
  // --bam_rg / --bam_oq (fq_bamin.h (b'')): the wanted IDs as the tag kernel reads them, and what it writes per record; per unit and side the OQ offsets
  bool tags = false, sel_up = false;
  int use_oq = 0;
  std::vector<uint32_t> h_sel;
  DBuf<uint32_t> sel, roq, unsel, hasoq, oq[2];
  DBuf<uint64_t> uord, qord;
  void select(const fq_bam_select_t *sl) {       // (before the first chunk)
    pack_bam_ids(sl, &h_sel);
    sel_up = false; use_oq = sl && sl->use_oq ? 1 : 0;
    tags = !h_sel.empty() || use_oq;
  }
};
struct BamChunk {                              // what the kernels found in one chunk's payload
  uint32_t n_rec = 0, n_kept = 0, n_units = 0;
  uint32_t chain_end = 0;                      // where the chain of whole records ends (the payload's end, or the record it cuts off)
  uint32_t carry_from = 0;                     // ... or in front of that, the last kept record of a paired stream when it has no mate yet
  uint32_t used_rec = 0;                       // records in front of carry_from
  int end_flag = FQB_SEG_OK, repairs = 0, paired = 0;
  uint64_t bad = FQB_NO_BAD, text_len[2] = {0, 0};
  uint64_t tag_bad = FQB_NO_BAD;               // (--bam_rg / --bam_oq) the tag kernel's first refusal, over all records of the payload
  uint32_t n_unsel = 0, n_oq = 0;              // ... of the records in front of carry_from: not selected; kept with an OQ value
};
// --collate: the records that wait for their mates, in HBM from chunk to chunk (two halves: a chunk's survivors are gathered from one into the other),
// with their offsets, name hashes and ordinals; and the scratch of the collation kernels
struct BamHeld {
  bool on = false;
  uint64_t mem = 0;                            // collate_mem: the most a half may hold (records + 24 bytes of arrays a record)
  DBuf<uint8_t> rec[2];
  DBuf<uint64_t> off[2], key[2], ord[2];
  DBuf<uint32_t> oq[2];                        // (--bam_oq) the held records' OQ offsets: 4 bytes more a record
  int cur = 0;
  uint32_t n = 0;                              // records held now
  uint64_t bytes = 0;
  int64_t peak_n = 0, peak_bytes = 0, orphans = 0;
  double ms[5] = {0, 0, 0, 0, 0};              // keys, sort, match, units, held gather
  uint32_t n_kept = 0;                         // (of the chunk under way: bam_collate_records -> bam_collate_hold)
  DBuf<uint64_t> hash, key_in, key_out, key_tmp, hoff, uidx, sidx, soff;
  DBuf<uint32_t> perm, perm_tmp, hist, st, mate, flag, surv, rlen;
  DBuf<uint8_t> from[2];
};
struct BamState {
  bool on = false;
  BamHeld K;
  int32_t n_ref = 0, paired = 0;
  uint64_t first_off = 0;                      // the first record's offset in the payload of the member the reader starts at
  bool first = true;
  BamWork W;
  DBuf<uint8_t> d_pay[2];                      // the chunks' payloads in turn: the raw carry of one leads the next
  int cur = 0;
  uint64_t carry_from = 0, carry_len = 0, ord0 = 0;
  int64_t records = 0, skipped = 0, repairs = 0, unselected = 0, oq_records = 0, empty_chunks = 0;
  double ms_starts = 0, ms_pairs = 0, ms_fill = 0, ms_tags = 0;
  double pay_total = 0, text0_total = 0;
};
}  // namespace

struct fq_frontend {
  BamState bam;
  int device = 0, n_files = 0, slot_mode = FQ_FASTQ_SLOTS_REUSED, batch_pairs = 262144;
  int64_t chunk_pairs = 16 * 262144;
  int max_len = 160;                           // rows the aligner sizes: a longer read ends the device's part
  FileSide f[2];
  fqdev::State *st = nullptr;                  // the producer's
  std::thread producer;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<fq_text_batch *> ready;
  bool slot_free[kSlots] = {true, true, true, true};
  uint64_t headroom_min = (uint64_t)64 << 20;   // least room kept in front of a chunk's new text for the carried text (FASTQUICK_FE_HEADROOM: tests)
  bool overlap = true;                         // the next chunk's members are inflated beside this chunk's kernels (FASTQUICK_FE_OVERLAP=0: one after the other)
  bool done = false, fallback = false, stop = false;
  std::string err;
  int rc = FQ_OK;
  fq_text_batch batch[kSlots];
  DBuf<FqTextRec> d_rec[kSlots];
  DBuf<uint64_t> d_head[kSlots];
  DBuf<uint16_t> d_hlen[kSlots];
  DBuf<char> d_names[kSlots];
  HBuf<uint32_t> h_stat;
  int max_name_ever = 0, min_name_ever = INT32_MAX;
  int64_t pairs_done = 0;
  int next_slot = 0;
  // totals (fq_frontend_stats)
  double ms_inflate = 0, ms_tokenise = 0, ms_lines = 0, ms_records = 0, ms_slots = 0;
  int64_t n_members = 0, n_refused = 0, text_bytes = 0, comp_bytes = 0, n_launch_inflate = 0, n_chunks = 0;
  double ms_wait_reader = 0, ms_wait_slot = 0;  // the producer's waits: for a chunk's compressed bytes; for a batch slot the caller still holds
  ~fq_frontend();
};

namespace {

// A piece of the file into (pinned) memory on several threads: a read from the page cache is a memcpy by the kernel, 8-12 GB/s on one
// thread -- slower than the device inflates what it brings.  Returns the bytes read from `off` on (short only at the end of the file).
ssize_t pread_threads(int fd, uint8_t *dst, size_t len, off_t off, int threads) {
  auto whole = [fd](uint8_t *d, size_t n, off_t o) -> ssize_t {
    size_t done = 0;
    while (done < n) {
      const ssize_t g = pread(fd, d + done, n - done, o + (off_t)done);
      if (g < 0) { if (errno == EINTR) continue; return -1; }
      if (g == 0) break;
      done += (size_t)g;
    }
    return (ssize_t)done;
  };
  const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, threads), len >> 22));
  if (nt == 1) return whole(dst, len, off);
  const size_t per = ((len + nt - 1) / nt + 4095) & ~(size_t)4095;
  std::vector<ssize_t> got((size_t)nt, 0);
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t)
    th.emplace_back([&, t] { const size_t lo = per * t; got[(size_t)t] = lo < len ? whole(dst + lo, std::min(per, len - lo), off + (off_t)lo) : 0; });
  got[0] = whole(dst, std::min(per, len), off);
  for (auto &x : th) x.join();
  ssize_t total = 0;
  for (int t = 0; t < nt; ++t) {
    if (got[(size_t)t] < 0) return -1;
    total += got[(size_t)t];
    if ((size_t)got[(size_t)t] < std::min(per, len - std::min(len, per * t))) break;      // the file ended inside this slice
  }
  return total;
}

// ---- reader thread: the next chunk's compressed bytes -> pinned staging -> HBM, with the member table -------------------------------
void reader_main(fq_frontend *fe, int e) {
  FileSide &F = fe->f[e];
  if (fqdev::bind(F.st)) { std::lock_guard<std::mutex> lk(F.mu); for (int k = 0; k < 3; ++k) { F.chunk[k].err = "no device"; F.filled[k] = true; } F.cv.notify_all(); return; }
  for (int k = 0;; k = (k + 1) % 3) {
    uint64_t want;
    {
      std::unique_lock<std::mutex> lk(F.mu);
      F.cv.wait(lk, [&] { return F.stop || !F.filled[k]; });
      if (F.stop) return;
      want = F.want_text;
    }
    // the stream's first chunks are short ones (an eighth, a quarter, a half of a chunk): the first batch is out after an eighth of the time,
    // and the kernels behind the reader have work while it reads
    static const int ramp = [] { const char *e = getenv("FASTQUICK_FE_RAMP"); const int v = e ? atoi(e) : 3; return v < 0 ? 0 : v > 5 ? 5 : v; }();      // (experiment knob: how many short chunks lead a stream)
    if (F.chunks_read < ramp) want = std::max<uint64_t>(want >> (ramp - F.chunks_read), (uint64_t)((double)fe->batch_pairs * F.text_per_record * 1.02) + (1u << 20));   // (a reference batch at least)
    if (fe->bam.on) { std::lock_guard<std::mutex> lk(F.mu); want = (uint64_t)((double)want * F.want_scale); }
    ++F.chunks_read;
    CompChunk &C = F.chunk[k];
    C.mem.clear(); C.comp_len = 0; C.text_len = 0; C.err.clear(); C.eof = false;
    // (sized in one go for what the chunk is expected to hold: growing the buffer under the uploads means waiting for them, and a hipFree waits for the device)
    (void)C.d_comp.ensure((size_t)std::min<double>((double)F.file_size - (double)F.file_off + (double)F.tail.size(), (double)want * F.comp_ratio * 1.1) + 2 * kPiece);
    // pieces: [tail of the previous read | new bytes] -> whole members go to the device, the rest is the next tail
    uint64_t text = 0;
    size_t dev_at = 0;
    int pin_i = 0;
    bool pin_used[2] = {false, false};
    bool more = true;
    while (more && C.err.empty()) {
      HBuf<uint8_t> &P = F.pin[pin_i];
      size_t have = F.tail.size();
      if (pin_used[pin_i]) { if (fqdev::copy_wait(pin_i)) { C.err = "upload failed"; break; } pin_used[pin_i] = false; }   // (the upload that last read this buffer)
      if (!P.ensure(have + kPiece + (1 << 17))) { C.err = "out of pinned host memory"; break; }
      if (have) memcpy(P.p, F.tail.data(), have);
      F.tail.clear();
      if (!F.file_eof && have < kPiece) {                    // (a long tail -- the rest of a piece whose chunk was full -- is used up first)
        const auto t0 = std::chrono::steady_clock::now();
        const ssize_t got = pread_threads(F.fd, P.p + have, kPiece, (off_t)F.file_off, F.read_threads);
        F.ms_read += ms_since(t0);
        if (got < 0) { C.err = "read error"; break; }
        if (got == 0) F.file_eof = true;
        F.file_off += got;
        have += (size_t)got;
      }
      // whole members of the piece
      size_t at = 0;
      while (have - at >= 18) {
        size_t hdr = 0;
        const size_t sz = bgzf_member(P.p + at, have - at, &hdr);
        if (sz == 0 || sz < hdr + 8) { C.err = "not a BGZF member at a member boundary (a bgzip file followed by something else?)"; break; }
        if (have - at < sz) break;
        const uint32_t isize = le32(P.p + at + sz - 4);
        if (isize) {
          FqzMember m{};
          m.in_off = dev_at + at + hdr; m.in_len = (uint32_t)(sz - hdr - 8); m.out_off = (uint32_t)text; m.out_len = isize; m.crc = le32(P.p + at + sz - 8);
          C.mem.push_back(m);
          text += isize;
        }
        at += sz;
        if (text >= want || text >= kMaxText) { more = false; break; }
      }
      if (!C.err.empty()) break;
      // the members' bytes go up; what is behind them waits for the next piece
      if (at) {
        if (C.d_comp.cap < dev_at + at + 2048) {               // (the uploads so far land before the buffer moves)
          for (int i = 0; i < 2; ++i) if (pin_used[i] && fqdev::copy_wait(i)) C.err = "upload failed";
          if (!C.err.empty()) break;
        }
        if (!C.d_comp.ensure_keep(dev_at + at + 2048, dev_at)) { C.err = "out of device memory"; break; }
        // (on the copy stream, with an event per staging buffer: the next piece is read while this one goes up)
        const auto t0 = std::chrono::steady_clock::now();
        if (fqdev::h2d_copy(C.d_comp.p + dev_at, P.p, at) || fqdev::copy_record(pin_i)) { C.err = "upload failed"; break; }
        pin_used[pin_i] = true;
        F.ms_upload += ms_since(t0);
        dev_at += at;
      }
      F.tail.assign(P.p + at, P.p + have);
      if (more && F.file_eof) {                              // the file has ended: every whole member has been taken, nothing may be left
        if (!F.tail.empty()) C.err = "truncated BGZF member at the end of the file";
        more = false;
      }
      pin_i ^= 1;
    }
    {
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; i < 2; ++i) if (pin_used[i] && fqdev::copy_wait(i) && C.err.empty()) C.err = "upload failed";
      F.ms_upload += ms_since(t0);
    }
    if (C.err.empty()) {
      C.file_off_end = F.file_off - (int64_t)F.tail.size();      // the first byte of the file that is not in this chunk
      C.comp_len = dev_at;
      C.text_len = text;
      if (text > (1u << 20)) F.comp_ratio = (double)dev_at / (double)text;
      C.eof = F.file_eof && F.tail.empty();
      if (!C.d_mem.ensure(C.mem.size() + 1) || !C.d_status.ensure(C.mem.size() + 1)) C.err = "out of device memory";
      if (C.err.empty() && dev_at && (fqdev::dzero(C.d_comp.p + dev_at, 1024) || fqdev::sync())) C.err = "upload failed";
    }
    const bool done = !C.err.empty() || C.eof;
    {
      std::lock_guard<std::mutex> lk(F.mu);
      F.filled[k] = true;
    }
    F.cv.notify_all();
    if (done) return;
  }
}

// Members the device refused: the host's decoder, then zlib, whose verdict stands.  text: what the members' out_off count from.
int host_inflate_refused(CompChunk &C, uint8_t *text, const std::string &path, int64_t *refused, std::string *err) {
  std::vector<uint32_t> status(C.mem.size());
  if (fqdev::d2h(status.data(), C.d_status.p, status.size() * 4) || fqdev::sync()) { *err = fqdev::last_error(); return FQ_ENODEV; }
  std::unique_ptr<fqz::Inflater> fz;
  std::vector<uint8_t> tmp, cbytes;
  for (size_t k = 0; k < status.size(); ++k) {
    if (status[k] == FQZ_OK) continue;
    ++*refused;
    const FqzMember &m = C.mem[k];
    cbytes.resize(m.in_len + 8);
    if (fqdev::d2h(cbytes.data(), C.d_comp.p + m.in_off, m.in_len) || fqdev::sync()) { *err = fqdev::last_error(); return FQ_ENODEV; }
    const uint8_t *src = cbytes.data();
    tmp.resize(m.out_len);
    bool ok = false;
    if (!fz) fz.reset(new fqz::Inflater);
    if (fqz::inflate_raw(*fz, src, m.in_len, tmp.data(), m.out_len)) ok = fqz::crc32(tmp.data(), m.out_len) == m.crc;
    else {
      z_stream zs;
      memset(&zs, 0, sizeof zs);
      if (inflateInit2(&zs, -15) == Z_OK) {
        zs.next_in = const_cast<Bytef *>(src); zs.avail_in = m.in_len; zs.next_out = tmp.data(); zs.avail_out = m.out_len;
        const int zr = inflate(&zs, Z_FINISH);
        ok = zr == Z_STREAM_END && zs.avail_out == 0 && (uint32_t)crc32(crc32(0L, Z_NULL, 0), tmp.data(), m.out_len) == m.crc;
        inflateEnd(&zs);
      }
    }
    if (!ok) { *err = path + ": corrupt BGZF member (inflate or CRC failed)"; return FQ_EIO; }
    if (fqdev::h2d(text + m.out_off, tmp.data(), m.out_len) || fqdev::sync()) { *err = fqdev::last_error(); return FQ_ENODEV; }
  }
  return FQ_OK;
}

// ---- BAM input: records of a payload in HBM -> the two FASTQ texts (kernels: fq_bamin.h) ------------------------------------------------
std::string bam_bad_message(uint64_t bad) {
  const unsigned long long ord = (unsigned long long)fqb_bad_ord(bad);
  const char *what = "is refused";
  switch ((int)fqb_bad_kind(bad)) {
    case FQB_BAD_MIXED: what = "paired and single-end records are mixed in one stream"; break;
    case FQB_BAD_LSEQ0: what = "a record without bases (l_seq == 0)"; break;
    case FQB_BAD_FIELDS: what = "the record's fields do not fit its block_size"; break;
    case FQB_BAD_NAME: what = "a read name byte outside 0x21..0x7e (or an empty name)"; break;
    case FQB_BAD_MATES: what = "mates are not adjacent: collate the file by name first (the two records are not a first and a second mate)"; break;
    case FQB_BAD_NAMES: what = "mates are not adjacent: collate the file by name first (the two records' names differ)"; break;
    case FQB_BAD_DUP: what = "a second record of this name and side before the mate of the first"; break;
    case FQB_BAD_AUX: what = "auxiliary fields cannot be walked (an unknown type, a value beyond the record, a Z / H value without NUL, stray bytes, or an RG / OQ tag that is not of type Z)"; break;
    case FQB_BAD_OQ: what = "OQ does not fit the read (its length is not l_seq, or a byte lies outside 0x21..0x7e)"; break;
  }
  return "BAM record " + std::to_string(ord) + ": " + what;
}
#define FQB_TRY(x) do { if (x) { *err = fqdev::last_error(); return FQ_ENODEV; } } while (0)
// Kernel (a) and the first of (b) over pay[0, n): the chain of records from rec0, cut at `cuts` (the members' starts behind rec0); who is kept, and the kept
// records' indices -- what bam_records and its collating sibling share.  *pb: the pair kernels' arguments as far as they are known here.
int bam_chain_kept(BamWork &W, const uint8_t *d_pay, uint32_t n, uint32_t rec0, const std::vector<uint32_t> &cuts, int32_t n_ref, uint64_t ord0, BamChunk *R, FqBamPairArgs *pb, std::string *err) {
  // ---- (a) the members' guesses ...
  W.h_seg.clear();
  W.h_seg.push_back(rec0);
  for (uint32_t c : cuts) if (c > rec0 && c < n) W.h_seg.push_back(c);
  const uint32_t S = (uint32_t)W.h_seg.size();
  W.h_seg.push_back(n);
  W.h_res.assign((size_t)4 * S, 0);
  if (!W.seg.ensure(S + 1) || !W.res.ensure((size_t)4 * S) || !W.base.ensure(S + 2)) { *err = "out of device memory (BAM records)"; return FQ_ENOMEM; }
  FqBamChainArgs a{};
  a.pay = d_pay; a.n = n; a.seg = W.seg.p; a.n_seg = S; a.n_ref = n_ref; a.first = W.res.p; a.last_next = W.res.p + S; a.count = W.res.p + 2 * (size_t)S; a.flag = W.res.p + 3 * (size_t)S;
  a.base = W.base.p;
  uint32_t *first = W.h_res.data(), *last_next = first + S, *count = first + 2 * (size_t)S, *flag = first + 3 * (size_t)S;
  fqdev::time_begin(4);
  FQB_TRY(fqdev::h2d(W.seg.p, W.h_seg.data(), 4 * (size_t)(S + 1)) || fqdev::launch_bam_guess(a) || fqdev::d2h(W.h_res.data(), W.res.p, 16 * (size_t)S) || fqdev::sync());
  // ---- ... held to the chain: member k's walk stands only if it began where the chain enters k
  uint32_t p = rec0, k = 0;
  int relaunches = 0;
  bool ended = false;
  while (k < S) {
    if (first[k] != p) {
      ++R->repairs;
      if (++relaunches > FQB_MAX_REPAIRS) {       // too many wrong guesses: one thread walks the rest, and every member from k on holds the chain's values
        FQB_TRY(fqdev::launch_bam_rewalk(a, k, p, 1) || fqdev::d2h(W.h_res.data(), W.res.p, 16 * (size_t)S) || fqdev::sync());
        relaunches = INT32_MIN;
      } else {
        FQB_TRY(fqdev::launch_bam_rewalk(a, k, p, 0) || fqdev::d2h(first + k, a.first + k, 4) || fqdev::d2h(last_next + k, a.last_next + k, 4) || fqdev::d2h(count + k, a.count + k, 4) ||
                fqdev::d2h(flag + k, a.flag + k, 4) || fqdev::sync());
      }
      if (first[k] != p) { *err = "BAM records: the walk of a member did not start where it was told to"; return FQ_EIO; }
    }
    p = last_next[k];
    if (flag[k] != FQB_SEG_OK) { R->end_flag = (int)flag[k]; ended = true; }
    if (p >= n) ended = true;
    ++k;
    // members the chain jumps over (inside one record), or behind its end, hold no start -- whatever they guessed
    while (k < S && (ended || W.h_seg[k + 1] <= p)) {
      if (first[k] != FQB_NONE) { if (!ended) ++R->repairs; first[k] = FQB_NONE; last_next[k] = FQB_NONE; count[k] = 0; flag[k] = FQB_SEG_OK; }
      ++k;
    }
  }
  R->chain_end = R->carry_from = p;
  uint64_t total = 0;
  FQB_TRY(fqdev::h2d(W.res.p, W.h_res.data(), 16 * (size_t)S) || fqdev::launch_scan(a.count, W.base.p, S) || fqdev::d2h(&total, W.base.p + S, 8) || fqdev::sync());
  if (total > 0x7fffffffull) { *err = "more than 2^31 BAM records in one chunk"; return FQ_ELIMIT; }
  R->n_rec = R->used_rec = (uint32_t)total;
  if (!W.starts.ensure(total + 1) || !W.kept.ensure(total + 1) || !W.kord.ensure(total + 2) || !W.kidx.ensure(total + 1) || !W.bad.ensure(2)) { *err = "out of device memory (BAM records)"; return FQ_ENOMEM; }
  a.starts = W.starts.p;
  FQB_TRY(fqdev::launch_bam_starts(a));
  fqdev::time_end(4);
  // ---- (b) kept records, pairs, lengths
  if (W.tags) {                                  // (b''; its buffers and the IDs first: an allocation inside a timed region counts as that region's)
    const size_t nr = (size_t)R->n_rec;
    if (!W.roq.ensure(nr + 1) || !W.unsel.ensure(nr + 1) || !W.hasoq.ensure(nr + 1) || !W.uord.ensure(nr + 2) || !W.qord.ensure(nr + 2) || (!W.h_sel.empty() && !W.sel.ensure(W.h_sel.size()))) { *err = "out of device memory (BAM records)"; return FQ_ENOMEM; }
    if (!W.h_sel.empty() && !W.sel_up) { FQB_TRY(fqdev::h2d(W.sel.p, W.h_sel.data(), 4 * W.h_sel.size()) || fqdev::sync()); W.sel_up = true; }
  }
  fqdev::time_begin(5);
  FqBamPairArgs &b = *pb;
  b = FqBamPairArgs();
  b.pay = d_pay; b.starts = W.starts.p; b.n_rec = R->n_rec; b.kept = W.kept.p; b.kord = W.kord.p; b.kidx = W.kidx.p; b.ord0 = ord0; b.bad = W.bad.p;
  uint64_t n_kept = 0;
  if (W.tags) {                                  // (b''): who is kept says the walk of the auxiliary fields (timing id 12)
    FqBamTagArgs t{};
    t.pay = d_pay; t.starts = W.starts.p; t.n_rec = R->n_rec; t.ord0 = ord0; t.sel = W.h_sel.empty() ? nullptr : W.sel.p; t.use_oq = W.use_oq;
    t.kept = W.kept.p; t.roq = W.roq.p; t.unsel = W.unsel.p; t.hasoq = W.hasoq.p; t.bad = W.bad.p + 1;
    const uint64_t no_bad = FQB_NO_BAD;
    FQB_TRY(fqdev::h2d(W.bad.p + 1, &no_bad, 8));
    fqdev::time_begin(12);
    FQB_TRY(fqdev::launch_bam_tags(t));
    fqdev::time_end(12);
    FQB_TRY(fqdev::launch_scan(W.unsel.p, W.uord.p, R->n_rec) || fqdev::launch_scan(W.hasoq.p, W.qord.p, R->n_rec) || fqdev::d2h(&R->tag_bad, W.bad.p + 1, 8));
    if (W.use_oq) b.roq = W.roq.p;
  } else {
    FQB_TRY(fqdev::launch_bam_keep(b));
  }
  FQB_TRY(fqdev::launch_scan(W.kept.p, W.kord.p, R->n_rec) || fqdev::d2h(&n_kept, W.kord.p + R->n_rec, 8) || fqdev::sync());
  FQB_TRY(fqdev::launch_bam_kidx(b));
  R->n_kept = (uint32_t)n_kept;
  fqdev::time_end(5);
  return FQ_OK;
}
// (b'') behind the pairing: the counts over the records in front of carry_from, and the tag kernel's first refusal where its record lies there (a carried
// record is walked again with the next chunk, and what its unit may refuse it for comes first)
int bam_tag_results(BamWork &W, uint64_t ord0, BamChunk *R, std::string *err) {
  if (!W.tags || !R->n_rec) return FQ_OK;
  uint64_t u = 0, q = 0;
  FQB_TRY(fqdev::d2h(&u, W.uord.p + R->used_rec, 8) || fqdev::d2h(&q, W.qord.p + R->used_rec, 8) || fqdev::sync());
  R->n_unsel = (uint32_t)u; R->n_oq = (uint32_t)q;
  if (R->tag_bad != FQB_NO_BAD && fqb_bad_ord(R->tag_bad) < ord0 + R->used_rec) R->bad = std::min(R->bad, R->tag_bad);
  return FQ_OK;
}
// Kernels (a) and (b) over pay[0, n): the chain of records from rec0, cut at `cuts` (the members' starts behind rec0); who is kept, who pairs with
// whom, how long the texts are.  paired < 0: by the first kept record.  t_ms: kernel ids 4 (a) and 5 (b) of the bound state's timing.
int bam_records(BamWork &W, const uint8_t *d_pay, uint32_t n, uint32_t rec0, const std::vector<uint32_t> &cuts, int32_t n_ref, int paired, uint64_t ord0, BamChunk *R, std::string *err) {
  *R = BamChunk();
  R->paired = paired < 0 ? 0 : paired;
  R->chain_end = R->carry_from = n;
  if (rec0 >= n) return FQ_OK;
  FqBamPairArgs b{};
  if (const int rc = bam_chain_kept(W, d_pay, n, rec0, cuts, n_ref, ord0, R, &b, err)) return rc;
  const uint64_t n_kept = R->n_kept;
  // ---- (b), the rest: pairs, lengths
  fqdev::time_begin(5);
  auto start_of_kept = [&](uint32_t kk, uint32_t *idx, uint32_t *at) -> int {
    return fqdev::d2h(idx, W.kidx.p + kk, 4) || fqdev::sync() || fqdev::d2h(at, W.starts.p + *idx, 4) || fqdev::sync();
  };
  if (paired < 0 && n_kept) {
    uint32_t idx = 0, at = 0;
    uint8_t fl[2] = {0, 0};
    FQB_TRY(start_of_kept(0, &idx, &at) || fqdev::d2h(fl, d_pay + at + 18, 2) || fqdev::sync());
    R->paired = fl[0] & 1;
  }
  R->n_units = R->paired ? R->n_kept / 2 : R->n_kept;
  if (R->paired && (R->n_kept & 1)) {            // the last kept record has no mate in this payload
    uint32_t idx = 0, at = 0;
    FQB_TRY(start_of_kept(R->n_kept - 1, &idx, &at));
    R->carry_from = at; R->used_rec = idx;
  }
  const uint32_t U = R->n_units;
  const int sides = R->paired ? 2 : 1;
  for (int e = 0; e < sides; ++e) if (!W.src[e].ensure(U + 1) || !W.len[e].ensure(U + 1) || !W.off[e].ensure(U + 2) || (b.roq && !W.oq[e].ensure(U + 1))) { *err = "out of device memory (BAM records)"; return FQ_ENOMEM; }
  b.n_units = U; b.paired = R->paired;
  for (int e = 0; e < 2; ++e) { b.src[e] = W.src[e].p; b.len[e] = W.len[e].p; b.oq[e] = W.oq[e].p; }
  const uint64_t no_bad = FQB_NO_BAD;
  FQB_TRY(fqdev::h2d(W.bad.p, &no_bad, 8) || fqdev::launch_bam_units(b));
  for (int e = 0; e < sides; ++e) FQB_TRY(fqdev::launch_scan(W.len[e].p, W.off[e].p, U) || fqdev::d2h(&R->text_len[e], W.off[e].p + U, 8));
  FQB_TRY(fqdev::d2h(&R->bad, W.bad.p, 8) || fqdev::sync());
  fqdev::time_end(5);
  return bam_tag_results(W, ord0, R, err);
}
// Kernel (c): the texts of the chunk's units at text[e] (timing id 6)
int bam_fill(BamWork &W, const uint8_t *d_pay, const BamChunk &R, uint8_t *const text[2], std::string *err, const BamHeld *K = nullptr) {
  FqBamFillArgs f{};
  f.pay = d_pay; f.n_units = R.n_units; f.n_sides = R.paired ? 2 : 1;
  for (int e = 0; e < f.n_sides; ++e) { f.src[e] = W.src[e].p; f.off[e] = W.off[e].p; f.text[e] = text[e]; f.total[e] = R.text_len[e]; }
  if (W.tags && W.use_oq) { f.oq[0] = W.oq[0].p; f.oq[1] = W.oq[1].p; }      // (--bam_oq: where a side's record has an OQ value, its quality line is that)
  if (K) { f.held = K->rec[K->cur].p; f.hoff = K->off[K->cur].p; f.from[0] = K->from[0].p; f.from[1] = K->from[1].p; }      // (collation: a side's record lies in the payload or in the held store)
  fqdev::time_begin(6);
  FQB_TRY(fqdev::launch_bam_fill(f));
  fqdev::time_end(6);
  return FQ_OK;
}

// ---- collation (--collate; fq_bamin.h (b')): in place of bam_records' pairing, mates are matched by name across the stream ----
FqBamCollateArgs collate_args(BamWork &W, BamHeld &K, const uint8_t *d_pay, uint64_t ord0) {
  FqBamCollateArgs c{};
  c.pay = d_pay; c.starts = W.starts.p; c.kidx = W.kidx.p; c.n_kept = K.n_kept; c.ord0 = ord0;
  c.held = K.rec[K.cur].p; c.hoff = K.off[K.cur].p; c.hkey = K.key[K.cur].p; c.hord = K.ord[K.cur].p; c.n_held = K.n;
  c.n = K.n + K.n_kept; c.mask = fqc_mask(fqdev::bam_hash_bits());
  c.hash = K.hash.p; c.key = K.key_in.p; c.st = K.st.p; c.mate = K.mate.p; c.skey = K.key_out.p; c.perm = K.perm.p; c.flag = K.flag.p; c.uidx = K.uidx.p;
  for (int e = 0; e < 2; ++e) { c.from[e] = K.from[e].p; c.src[e] = W.src[e].p; c.len[e] = W.len[e].p; }
  c.bad = W.bad.p; c.surv = K.surv.p; c.rlen = K.rlen.p; c.sidx = K.sidx.p; c.soff = K.soff.p;
  c.nheld = K.rec[K.cur ^ 1].p; c.noff = K.off[K.cur ^ 1].p; c.nkey = K.key[K.cur ^ 1].p; c.nord = K.ord[K.cur ^ 1].p;
  if (W.tags && W.use_oq) { c.roq = W.roq.p; c.hoq = K.oq[K.cur].p; c.noq = K.oq[K.cur ^ 1].p; c.oq[0] = W.oq[0].p; c.oq[1] = W.oq[1].p; }
  return c;
}
// The collating sibling of bam_records, for a paired stream: kernel (a) and who is kept as there; then the candidates -- the held records, then the
// chunk's kept records -- are keyed by their names' hashes, sorted, matched run by run, and the completing records scanned into units.  Nothing but
// the record the payload's end cuts off is carried raw: a kept record without its mate is held (bam_collate_hold, behind the fill).  Timing ids 7-10.
int bam_collate_records(BamWork &W, BamHeld &K, const uint8_t *d_pay, uint32_t n, uint32_t rec0, const std::vector<uint32_t> &cuts, int32_t n_ref, uint64_t ord0, BamChunk *R, std::string *err) {
  *R = BamChunk();
  R->paired = 1;
  R->chain_end = R->carry_from = n;
  K.n_kept = 0;
  if (rec0 >= n) return FQ_OK;
  FqBamPairArgs b{};
  if (const int rc = bam_chain_kept(W, d_pay, n, rec0, cuts, n_ref, ord0, R, &b, err)) return rc;
  K.n_kept = R->n_kept;
  if (!K.n_kept) return bam_tag_results(W, ord0, R, err);      // (no candidate of this chunk: what is held stays as it is)
  const uint64_t N64 = (uint64_t)K.n + K.n_kept;
  if (N64 > 0x7fffffffull) { *err = "more than 2^31 BAM records waiting for their mates"; return FQ_ELIMIT; }
  const uint32_t N = (uint32_t)N64, tiles = fq_sort_tiles(N);
  if (!K.hash.ensure(N) || !K.key_in.ensure(N) || !K.key_out.ensure(N) || !K.key_tmp.ensure(N) || !K.perm.ensure(N) || !K.perm_tmp.ensure(N) || !K.st.ensure(N) || !K.mate.ensure(N) ||
      !K.hist.ensure((size_t)FQ_SORT_DIGITS * tiles + 1) || !K.hoff.ensure((size_t)FQ_SORT_DIGITS * tiles + 2) || !K.flag.ensure(K.n_kept + 1) || !K.uidx.ensure(K.n_kept + 2) ||
      !K.surv.ensure(N + 1) || !K.rlen.ensure(N + 1) || !K.sidx.ensure(N + 2) || !K.soff.ensure(N + 2) || !W.bad.ensure(2)) { *err = "out of device memory (BAM collation)"; return FQ_ENOMEM; }
  FqBamCollateArgs c = collate_args(W, K, d_pay, ord0);
  const uint64_t no_bad = FQB_NO_BAD;
  fqdev::time_begin(7);
  FQB_TRY(fqdev::h2d(W.bad.p, &no_bad, 8) || fqdev::launch_bam_ckeys(c));
  fqdev::time_end(7);
  fqdev::time_begin(8);
  const FqSortScratch sc{K.key_tmp.p, K.perm_tmp.p, K.hist.p, K.hoff.p};
  FQB_TRY(fqdev::launch_sort_pairs(K.key_in.p, N, fqdev::bam_hash_bits(), K.key_out.p, K.perm.p, sc));
  fqdev::time_end(8);
  fqdev::time_begin(9);
  FQB_TRY(fqdev::launch_bam_cmatch(c));
  fqdev::time_end(9);
  fqdev::time_begin(10);
  uint64_t n_units = 0;
  FQB_TRY(fqdev::launch_scan(K.flag.p, K.uidx.p, K.n_kept) || fqdev::d2h(&n_units, K.uidx.p + K.n_kept, 8) || fqdev::sync());
  const uint32_t U = R->n_units = (uint32_t)n_units;
  for (int e = 0; e < 2; ++e) if (!W.src[e].ensure(U + 1) || !W.len[e].ensure(U + 1) || !W.off[e].ensure(U + 2) || !K.from[e].ensure(U + 1) || (W.tags && W.use_oq && !W.oq[e].ensure(U + 1))) { *err = "out of device memory (BAM collation)"; return FQ_ENOMEM; }
  c = collate_args(W, K, d_pay, ord0);
  FQB_TRY(fqdev::launch_bam_cunits(c));
  for (int e = 0; e < 2; ++e) FQB_TRY(fqdev::launch_scan(W.len[e].p, W.off[e].p, U) || fqdev::d2h(&R->text_len[e], W.off[e].p + U, 8));
  FQB_TRY(fqdev::d2h(&R->bad, W.bad.p, 8) || fqdev::sync());
  fqdev::time_end(10);
  return bam_tag_results(W, ord0, R, err);
}
// Behind the chunk's fill: the candidates that still wait -- old held records and new ones, in ordinal order -- are gathered into the other half of the
// held store, a wavefront a record.  FQ_ELIMIT where they would take more than collate_mem.  Timing id 11.
int bam_collate_hold(BamWork &W, BamHeld &K, const uint8_t *d_pay, uint64_t ord0, std::string *err) {
  if (!K.n_kept) return FQ_OK;
  const uint32_t N = K.n + K.n_kept;
  FqBamCollateArgs c = collate_args(W, K, d_pay, ord0);
  uint64_t count = 0, bytes = 0;
  fqdev::time_begin(11);
  FQB_TRY(fqdev::launch_bam_cmark(c) || fqdev::launch_scan(K.surv.p, K.sidx.p, N) || fqdev::launch_scan(K.rlen.p, K.soff.p, N) || fqdev::d2h(&count, K.sidx.p + N, 8) || fqdev::d2h(&bytes, K.soff.p + N, 8) ||
          fqdev::sync());
  const bool with_oq = W.tags && W.use_oq;
  const uint64_t total = bytes + (with_oq ? 28 : 24) * count;
  if (total > K.mem) {
    *err = "BAM record " + std::to_string(ord0) + ": behind the chunk that begins here " + std::to_string(count) + " records wait for their mates, " + std::to_string(total) +
           " bytes: more than --collate_mem " + std::to_string(K.mem) + " (a file with many mates far apart, or many records without a mate)";
    return FQ_ELIMIT;
  }
  const int o = K.cur ^ 1;
  if (!K.rec[o].ensure((size_t)bytes + 1) || !K.off[o].ensure(count + 1) || !K.key[o].ensure(count + 1) || !K.ord[o].ensure(count + 1) || (with_oq && !K.oq[o].ensure(count + 1))) { *err = "out of device memory (BAM records waiting for their mates)"; return FQ_ENOMEM; }
  c = collate_args(W, K, d_pay, ord0);
  FQB_TRY(fqdev::launch_bam_chold(c) || fqdev::sync());
  fqdev::time_end(11);
  K.cur = o; K.n = (uint32_t)count; K.bytes = total; K.n_kept = 0;
  K.peak_n = std::max<int64_t>(K.peak_n, (int64_t)count); K.peak_bytes = std::max<int64_t>(K.peak_bytes, (int64_t)total);
  return FQ_OK;
}

// One chunk's inflation, started one chunk ahead of the kernels that read its text (producer_main)
struct Ahead {
  bool open = false;                // a batch slot is taken and the members of the files that still have some are being inflated
  int slot = -1, comp_k = -1;
  bool has[2] = {false, false};     // the file had a compressed chunk for this one
  uint64_t H[2] = {0, 0};           // where its new text begins in d_text[slot] (a multiple of 256: the carried text goes in front of it)
};

// BAM input, one chunk: the one compressed side's members inflated into a payload buffer behind the previous chunk's raw carry (the record the
// payload's end cut off; a last kept record without its mate), the records transcoded into both sides' d_text[slot] at their H.  Everything runs
// on the main stream and is waited for: BAM chunks run one after the other (the text lengths are known only when kernel (b) has run).  The
// sides' CompChunk of this turn are then made to say what the FASTQ path reads from them: text_len, eof, no member left to look at.
int bam_chunk(fq_frontend *fe, CompChunk &C, int slot, Ahead &next, std::string *err) {
  BamState &S = fe->bam;
  FileSide &F0 = fe->f[0];
  const int NF = fe->n_files;
  if (!C.err.empty()) { *err = F0.path + ": " + C.err; return FQ_EIO; }
  const uint64_t carry = S.carry_len, P0 = (carry + 255) & ~(uint64_t)255, n64 = P0 + C.text_len;
  if (n64 > 0xfff00000ull) { *err = "a chunk's BAM payload exceeds 4 GiB"; return FQ_ELIMIT; }
  const uint32_t n = (uint32_t)n64;
  DBuf<uint8_t> &buf = S.d_pay[S.cur ^ 1];
  if (!buf.ensure((size_t)n + 4096)) { *err = "out of device memory (BAM payload)"; return FQ_ENOMEM; }
  if (carry) FQB_TRY(fqdev::d2d(buf.p + (P0 - carry), S.d_pay[S.cur].p + S.carry_from, (size_t)carry));
  int64_t refused = 0;
  if (!C.mem.empty()) {
    for (auto &m : C.mem) m.out_off += (uint32_t)P0;
    FqInflateArgs a{};
    a.comp = C.d_comp.p; a.mem = C.d_mem.p; a.n_mem = (int)C.mem.size(); a.out = buf.p; a.status = C.d_status.p; a.crc = fqdev::crc_const();
    if (!a.crc) { *err = fqdev::last_error(); return FQ_ENODEV; }
    FQB_TRY(fqdev::h2d(C.d_mem.p, C.mem.data(), C.mem.size() * sizeof(FqzMember)));
    fqdev::time_begin(0);
    FQB_TRY(fqdev::launch_inflate(a));
    fqdev::time_end(0);
    if (const int rc = host_inflate_refused(C, buf.p, F0.path, &refused, err)) return rc;
  }
  const uint32_t rec0 = (uint32_t)(P0 - carry + (S.first ? S.first_off : 0));
  S.first = false;
  std::vector<uint32_t> cuts;
  cuts.reserve(C.mem.size());
  for (const auto &m : C.mem) cuts.push_back(m.out_off);
  BamChunk R;
  const bool collate = S.K.on && S.paired;       // (a single-end stream has no mates to find: --collate changes nothing)
  if (const int rc = collate ? bam_collate_records(S.W, S.K, buf.p, n, rec0, cuts, S.n_ref, S.ord0, &R, err) : bam_records(S.W, buf.p, n, rec0, cuts, S.n_ref, S.paired, S.ord0, &R, err)) return rc;
  if (R.end_flag == FQB_SEG_CORRUPT) { *err = F0.path + ": BAM record " + std::to_string(S.ord0 + R.n_rec) + ": its block_size is not a record's"; return FQ_EIO; }
  if (R.bad != FQB_NO_BAD) { *err = F0.path + ": " + bam_bad_message(R.bad); return FQ_EIO; }
  if (C.eof && R.chain_end != n) { *err = F0.path + ": the stream ends inside a record (BAM record " + std::to_string(S.ord0 + R.n_rec) + ")"; return FQ_EIO; }
  if (C.eof && R.carry_from != n) { *err = F0.path + ": " + bam_bad_message(fqb_bad(S.ord0 + R.used_rec, FQB_BAD_MATES)) + " -- the last record has no mate"; return FQ_EIO; }
  uint8_t *text[2] = {nullptr, nullptr};
  for (int e = 0; e < NF; ++e) {
    FileSide &F = fe->f[e];
    const uint64_t H = ((uint64_t)std::max<double>((double)fe->headroom_min, fe->headroom_min ? 1.5 * (double)fe->batch_pairs * F.text_per_record : 0.0) + 255) & ~(uint64_t)255;
    next.H[e] = H; next.has[e] = true;
    if (H + R.text_len[e] > 0xfff00000ull) { *err = "a chunk's text exceeds 4 GiB"; return FQ_ELIMIT; }
    if (!F.d_text[slot].ensure((size_t)(H + R.text_len[e]) + 4096)) { *err = "out of device memory (text)"; return FQ_ENOMEM; }
    text[e] = F.d_text[slot].p + H;
  }
  if (const int rc = bam_fill(S.W, buf.p, R, text, err, collate ? &S.K : nullptr)) return rc;
  FQB_TRY(fqdev::sync());
  if (collate) {
    if (const int rc = bam_collate_hold(S.W, S.K, buf.p, S.ord0, err)) { *err = F0.path + ": " + *err; return rc; }
    if (C.eof) S.K.orphans = S.K.n;               // what still waits at the end of the stream has no mate in it
    if (C.eof && S.K.n && S.W.tags && S.W.use_oq) {      // (... and its OQ values were read by nobody)
      std::vector<uint32_t> hoq(S.K.n);
      FQB_TRY(fqdev::d2h(hoq.data(), S.K.oq[S.K.cur].p, 4 * (size_t)S.K.n) || fqdev::sync());
      for (uint32_t v : hoq) if (v) --S.oq_records;
    }
  }
  // what the stream keeps
  S.cur ^= 1; S.carry_from = R.carry_from; S.carry_len = n - R.carry_from;
  S.ord0 += R.used_rec; S.records += R.used_rec; S.skipped += (collate ? (int64_t)R.n_rec - (int64_t)R.n_kept : (int64_t)R.used_rec - (int64_t)R.n_units * (R.paired ? 2 : 1)) - (int64_t)R.n_unsel; S.repairs += R.repairs;
  S.unselected += R.n_unsel; S.oq_records += R.n_oq;
  if (R.n_rec && !R.n_kept) ++S.empty_chunks;
  S.pay_total += (double)(R.carry_from - rec0); S.text0_total += (double)R.text_len[0];
  fe->n_members += (int64_t)C.mem.size(); fe->n_refused += refused; fe->comp_bytes += (int64_t)C.comp_len; fe->text_bytes += (int64_t)(R.text_len[0] + R.text_len[1]);
  // (under collation a chunk's text says nothing about its payload -- it may complete no pair at all: the open's estimate of the scale stands)
  if (S.text0_total > 0 && !collate) { std::lock_guard<std::mutex> lk(F0.mu); F0.want_scale = S.pay_total / S.text0_total; }
  const bool eof = C.eof;
  for (int e = 0; e < NF; ++e) {
    CompChunk &D = fe->f[e].chunk[next.comp_k];
    D.mem.clear(); D.err.clear(); D.text_len = R.text_len[e]; D.eof = eof;
    if (eof) fe->f[e].all_launched = true;
  }
  return FQ_OK;
}

// the producer: chunk after chunk until the end of the stream, a failure, or something the device does not take.
// Two streams: the members of chunk j + 1 are inflated (aux stream) while chunk j's text is indexed, checked and keyed (main stream) -- the
// decoder is bound by the latency of its own dependent steps and leaves the memory system to the kernels beside it.  A chunk's text begins with
// what the chunk before it left over behind its last whole reference batch, and how much that is is known only when that chunk has been
// tokenised: the new text is inflated at a fixed distance H from the buffer's start and the carried text copied in front of it afterwards.
void producer_main(fq_frontend *fe) {
  auto finish = [&](int rc, const std::string &err, bool fallback) {
    std::lock_guard<std::mutex> lk(fe->mu);
    if (rc) { fe->rc = rc; fe->err = err; }
    fe->fallback = fallback;
    fe->done = true;
    fe->cv.notify_all();
  };
  if (fqdev::bind(fe->st)) { finish(FQ_ENODEV, "no device", false); return; }
  if (fe->overlap && fqdev::stream_aux(1)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }   // (creates the second stream)
  fqdev::stream_aux(0);
  const int NF = fe->n_files;
  const int B = fe->batch_pairs;
  const int n_slots = 2 * B;
  int comp_next = 0;                 // the compressed slot the next chunk's members are in
  int64_t n_started = 0, n_taken = 0;   // chunks whose inflation has been started / whose text has been taken up (their marks alternate)
  Ahead next;
  // Starts the next chunk's inflation.  block: wait for a batch slot and for the readers; otherwise only when both are there already.
  // Returns 1 started (or nothing is left to inflate: the chunk is its carried text), 0 not now, -1 failed / stopped (finish() has been called).
  auto start_ahead = [&](bool block) -> int {
    if (next.open) return 1;
    {
      const auto t0 = std::chrono::steady_clock::now();
      std::unique_lock<std::mutex> lk(fe->mu);
      if (!block && !(fe->stop || fe->slot_free[fe->next_slot])) return 0;
      fe->cv.wait(lk, [&] { return fe->stop || fe->slot_free[fe->next_slot]; });
      fe->ms_wait_slot += ms_since(t0);
      if (fe->stop) return -1;
    }
    CompChunk *Cs[2] = {nullptr, nullptr};
    for (int e = 0; e < NF; ++e) {
      FileSide &F = fe->f[e];
      if (F.all_launched) continue;
      const auto t0 = std::chrono::steady_clock::now();
      std::unique_lock<std::mutex> lk(F.mu);
      if (!block && !F.filled[comp_next]) return 0;
      F.cv.wait(lk, [&] { return F.stop || F.filled[comp_next]; });
      fe->ms_wait_reader += ms_since(t0);
      if (!F.filled[comp_next]) return -1;                   // (the front end is being closed in the middle of the stream)
      Cs[e] = &F.chunk[comp_next];
    }
    int slot;
    {
      std::lock_guard<std::mutex> lk(fe->mu);
      slot = fe->next_slot;
      fe->slot_free[slot] = false;
      fe->next_slot = (slot + 1) % kSlots;
    }
    next = Ahead();
    next.open = true; next.slot = slot; next.comp_k = comp_next;
    if (fe->bam.on) {
      if (Cs[0]) { std::string em; const int rc = bam_chunk(fe, *Cs[0], slot, next, &em); if (rc) { finish(rc, em, false); return -1; } }
      ++n_started;
      comp_next = (comp_next + 1) % 3;
      return 1;
    }
    FqInflateArgs ia[2] = {FqInflateArgs(), FqInflateArgs()};
    for (int e = 0; e < NF; ++e) {
      FileSide &F = fe->f[e];
      CompChunk *C = Cs[e];
      if (!C) continue;
      next.has[e] = true;
      if (!C->err.empty()) { finish(FQ_EIO, F.path + ": " + C->err, false); return -1; }
      if (C->eof) F.all_launched = true;
      // room in front of the new text for what the chunk before leaves over: a reference batch's worth and a half, 64 MB at least
      const uint64_t H = ((uint64_t)std::max<double>((double)fe->headroom_min, fe->headroom_min ? 1.5 * (double)B * F.text_per_record : 0.0) + 255) & ~(uint64_t)255;
      next.H[e] = H;
      if (H + C->text_len > 0xfff00000ull) { finish(FQ_ELIMIT, "a chunk's text exceeds 4 GiB", false); return -1; }
      if (!F.d_text[slot].ensure((size_t)(H + C->text_len) + 4096)) { finish(FQ_ENOMEM, "out of device memory (text)", false); return -1; }
      if (C->mem.empty()) continue;
      for (auto &m : C->mem) m.out_off += (uint32_t)H;       // (256-byte alignment of the buffer's base is what the decoder's stores rely on: the shift is in the members' offsets)
      FqInflateArgs &a = ia[e];
      a.comp = C->d_comp.p; a.mem = C->d_mem.p; a.n_mem = (int)C->mem.size(); a.out = F.d_text[slot].p; a.status = C->d_status.p;
    }
    if (ia[0].n_mem > 0 || ia[1].n_mem > 0) {
      // one launch for the two files' members: the last of a launch's rounds of wavefronts is the fuller for it
      if (fe->overlap) fqdev::stream_aux(1);
      bool bad = false;
      for (int e = 0; e < NF; ++e) {
        if (ia[e].n_mem <= 0) continue;
        CompChunk *C = Cs[e];
        bad = bad || fqdev::h2d(C->d_mem.p, C->mem.data(), C->mem.size() * sizeof(FqzMember));
        ia[e].crc = fqdev::crc_const();
        bad = bad || !ia[e].crc;
      }
      if (!bad) {
        fqdev::time_begin(0);
        bad = fqdev::launch_inflate2(ia[0], ia[1]) != 0;
        fqdev::time_end(0);
      }
      fqdev::stream_aux(0);
      if (bad) { finish(FQ_ENODEV, fqdev::last_error(), false); return -1; }
    }
    if (fe->overlap) { fqdev::stream_aux(1); const int rc = fqdev::stream_mark((int)(n_started & 1)); fqdev::stream_aux(0); if (rc) { finish(FQ_ENODEV, fqdev::last_error(), false); return -1; } }
    ++n_started;
    comp_next = (comp_next + 1) % 3;
    return 1;
  };
  for (;;) {
    // ---- this chunk: its members are being inflated already, or are started now ----
    if (start_ahead(true) < 0) return;
    const Ahead cur = next;
    next = Ahead();
    const int slot = cur.slot;
    fq_text_batch &TB = fe->batch[slot];
    TB = fq_text_batch();
    TB.slot = slot; TB.device = fe->device; TB.single_end = NF == 1; TB.batch_pairs = B; TB.row_cap = fe->max_len;
    uint32_t n_lines[2] = {0, 0};
    uint64_t n_text[2] = {0, 0};      // bytes of the chunk's view: [0, skip) in front of the text for the alignment, then carried text, then new text
    uint32_t skip[2] = {0, 0};
    uint64_t view[2] = {0, 0};        // where the view begins in d_text[slot] (a multiple of 16)
    bool at_eof[2] = {true, true};
    double t_ms[FQ_K_COUNT] = {0};
    uint64_t t_n[FQ_K_COUNT] = {0};
    if (fe->overlap && fqdev::stream_wait_mark((int)(n_taken & 1))) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
    ++n_taken;
    // ---- the carried text in front of the new text ----
    for (int e = 0; e < NF; ++e) {
      FileSide &F = fe->f[e];
      CompChunk *C = cur.has[e] ? &F.chunk[cur.comp_k] : nullptr;
      const uint64_t new_text = C ? C->text_len : 0;
      uint64_t H = C ? cur.H[e] : ((F.carry_len + 255) & ~(uint64_t)255);
      if (!C && !F.d_text[slot].ensure((size_t)(H + 4096))) { finish(FQ_ENOMEM, "out of device memory (text)", false); return; }
      if (C && F.carry_len > H) {
        // more was left over than there is room in front of the new text (reads of kilobytes; files whose records differ much in size): the new
        // text moves back, through a second buffer
        const uint64_t H2 = (F.carry_len + 255) & ~(uint64_t)255;
        DBuf<uint8_t> tmp;
        if (H2 + new_text > 0xfff00000ull) { finish(FQ_ELIMIT, "a chunk's text exceeds 4 GiB", false); return; }
        if (!tmp.ensure((size_t)new_text + 256) || fqdev::d2d(tmp.p, F.d_text[slot].p + H, (size_t)new_text) || fqdev::sync() ||
            !F.d_text[slot].ensure_keep((size_t)(H2 + new_text) + 4096, 0) || fqdev::d2d(F.d_text[slot].p + H2, tmp.p, (size_t)new_text) || fqdev::sync()) { finish(FQ_ENOMEM, "out of device memory (text)", false); return; }
        for (auto &m : C->mem) m.out_off += (uint32_t)(H2 - H);
        H = H2;
      }
      const uint64_t t0 = H - F.carry_len;
      view[e] = t0 & ~(uint64_t)15; skip[e] = (uint32_t)(t0 & 15);
      n_text[e] = skip[e] + F.carry_len + new_text;
      if (F.carry_len && fqdev::d2d(F.d_text[slot].p + t0, F.d_text[F.carry_slot].p + F.carry_off, (size_t)F.carry_len)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
      if (C) F.inflated_file_off = C->file_off_end;
      at_eof[e] = C ? C->eof : true;
    }
    // ---- members the device refused: the host's decoder, then zlib, whose verdict stands ----
    for (int e = 0; e < NF; ++e) {
      FileSide &F = fe->f[e];
      if (!cur.has[e]) continue;
      CompChunk &C = F.chunk[cur.comp_k];
      if (C.mem.empty()) continue;
      {
        std::string em;
        int64_t n_ref = 0;
        const int rc = host_inflate_refused(C, F.d_text[slot].p, F.path, &n_ref, &em);
        TB.refused += n_ref;
        if (rc) { finish(rc, em, false); return; }
      }
      TB.members += (int64_t)C.mem.size(); TB.comp_bytes += (int64_t)C.comp_len; TB.text_bytes += (int64_t)C.text_len;
    }
    // ---- the compressed slot is free again: the reader threads run up to two chunks ahead ----
    for (int e = 0; e < NF; ++e) {
      FileSide &F = fe->f[e];
      if (!cur.has[e]) continue;
      std::lock_guard<std::mutex> lk(F.mu);
      F.filled[cur.comp_k] = false;
      F.cv.notify_all();
    }
    // ---- the next chunk's members, beside this chunk's kernels (when its compressed bytes and a batch slot are there already) ----
    if (fe->overlap && start_ahead(false) < 0) return;
    // ---- line ends ----
    fqdev::time_begin(1);
    for (int e = 0; e < NF; ++e) {
      FileSide &F = fe->f[e];
      const size_t cap = (size_t)(4 * (fe->chunk_pairs + B) + 64);
      if (!F.d_nl.ensure(cap) || !F.d_stat.ensure(FQT_N_STAT + 8)) { finish(FQ_ENOMEM, "out of device memory (line index)", false); return; }
      uint8_t *T = F.d_text[slot].p + view[e];
      if (fqdev::dzero(T + n_text[e], 256)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
      if (fqdev::launch_nl_index(T, (uint32_t)n_text[e], skip[e], F.d_nl.p, (uint32_t)cap, F.d_stat.p + FQT_N_STAT)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
    }
    fqdev::time_end(1);
    if (!fe->h_stat.ensure(64)) { finish(FQ_ENOMEM, "out of pinned host memory", false); return; }
    for (int e = 0; e < NF; ++e) if (fqdev::copy_pinned(fe->h_stat.p + 32 * e, fe->f[e].d_stat.p + FQT_N_STAT, 4, 0)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
    if (fqdev::sync()) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
    for (int e = 0; e < NF; ++e) n_lines[e] = fe->h_stat.p[32 * e];
    // ---- how many pairs this chunk holds ----
    int64_t n = fe->chunk_pairs;
    bool all_eof = true;
    for (int e = 0; e < NF; ++e) {
      const size_t cap_lines = (size_t)(4 * (fe->chunk_pairs + B));
      n = std::min<int64_t>(n, (int64_t)(std::min<size_t>(n_lines[e], cap_lines) / 4));
      all_eof = all_eof && at_eof[e];
    }
    bool last = false;
    if (all_eof) {
      // the stream's end is in sight: every whole record that is left goes into this chunk when they fit it
      int64_t rest = INT64_MAX;
      for (int e = 0; e < NF; ++e) rest = std::min<int64_t>(rest, (int64_t)(n_lines[e] / 4));
      if (rest <= fe->chunk_pairs) { n = rest; last = true; }
    }
    if (!last) n = n / B * B;
    bool fall = false;
    // ---- records, keys (again after a cut: the rows of the second file begin at n) ----
    int n_rows = (int)(NF * n);
    while (n > 0) {
      n_rows = (int)(NF * n);
      if (!fe->d_rec[slot].ensure((size_t)n_rows + 1) || !fe->d_head[slot].ensure((size_t)n_rows * 3 + 8) || !fe->d_hlen[slot].ensure((size_t)n_rows + 8)) { finish(FQ_ENOMEM, "out of device memory (records)", false); return; }
      for (int e = 0; e < NF; ++e) {
        FileSide &F = fe->f[e];
        const uint32_t init[FQT_N_STAT] = {0xffffffffu, 0, 0xffffffffu, 0, 0, 0xffffffffu, 0, 0};
        if (fqdev::h2d(F.d_stat.p, init, sizeof init)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
        FqTokArgs a{};
        a.text = F.d_text[slot].p + view[e]; a.text0 = skip[e]; a.nl = F.d_nl.p; a.n_rec = (int)n; a.row0 = (int)(e * n); a.n_rows = n_rows; a.max_len = fe->max_len;
        a.rec = fe->d_rec[slot].p; a.head = fe->d_head[slot].p; a.hlen = fe->d_hlen[slot].p; a.stat = F.d_stat.p;
        fqdev::time_begin(2);
        if (fqdev::launch_tok_rec(a) || fqdev::launch_tok_pieces(a)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
        fqdev::time_end(2);
        if (fqdev::copy_pinned(fe->h_stat.p + 32 * e, F.d_stat.p, 4 * FQT_N_STAT, 0)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
      }
      if (fqdev::sync()) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
      int64_t first_bad = INT64_MAX;
      for (int e = 0; e < NF; ++e) if (fe->h_stat.p[32 * e + FQT_FIRST_BAD] != 0xffffffffu) first_bad = std::min<int64_t>(first_bad, (int64_t)fe->h_stat.p[32 * e + FQT_FIRST_BAD]);
      if (first_bad >= n) break;
      // a record the device does not take: its reference batch, and everything behind it, goes the host's way; the batches in front of it
      // are good (the same launch checked them)
      n = first_bad / B * B;
      fall = true; last = false;
    }
    if (n > 0) {
      // (min / max over the records that are in the chunk: the statistics above cover records [0, n_checked) of which the chunk may hold
      //  fewer after a cut -- a longer maximum only sizes a buffer more generously; lengths are told apart per row by the aligner)
      int min_len = INT32_MAX, max_len = 0, max_name = 0, min_name = INT32_MAX;
      for (int e = 0; e < NF; ++e) {
        min_name = std::min<int>(min_name, (int)std::min<uint32_t>(fe->h_stat.p[32 * e + FQT_MIN_NAME], 0x7fffffffu));
        min_len = std::min<int>(min_len, (int)std::min<uint32_t>(fe->h_stat.p[32 * e + FQT_MIN_LEN], 0x7fffffffu));
        max_len = std::max<int>(max_len, (int)fe->h_stat.p[32 * e + FQT_MAX_LEN]);
        max_name = std::max<int>(max_name, (int)fe->h_stat.p[32 * e + FQT_MAX_NAME]);
      }
      fe->max_name_ever = std::max(fe->max_name_ever, max_name);
      fe->min_name_ever = std::min(fe->min_name_ever, min_name);
      // (a cut chunk's statistics cover the records behind the cut too: at worst the general kernels run where the plain ones would have done)
      const bool plain_names = fe->slot_mode != FQ_FASTQ_SLOTS_REUSED || fe->min_name_ever == fe->max_name_ever;
      const bool all_long = min_len >= 96;
      const int name_stride = std::min(304, (fe->max_name_ever + 1 + 15) & ~15);
      TB.n_pairs = (int)n; TB.uniform_len = (!fall && min_len == max_len) ? max_len : 0; TB.max_len = max_len; TB.name_stride = name_stride;
      if (!fe->d_names[slot].ensure((size_t)n_rows * (size_t)name_stride + 64)) { finish(FQ_ENOMEM, "out of device memory (names)", false); return; }
      // ---- the read slots: bases behind short reads, names ----
      for (int e = 0; e < NF; ++e) {
        FileSide &F = fe->f[e];
        FqSlotArgs s{};
        s.text = F.d_text[slot].p + view[e]; s.rec = fe->d_rec[slot].p; s.n_rec = (int)n; s.row0 = (int)(e * n); s.n_rows = n_rows; s.g0 = F.records_done;
        s.n_slots = n_slots; s.mode = fe->slot_mode; s.slot_base = F.d_slot_base.p; s.slot_len = F.d_slot_len.p; s.slot_name = F.d_slot_name.p;
        s.head = fe->d_head[slot].p; s.names = fe->d_names[slot].p; s.name_stride = name_stride; s.stat = F.d_stat.p;
        s.all_long = all_long ? 1 : 0; s.plain_names = plain_names ? 1 : 0;
        fqdev::time_begin(3);
        if (fe->slot_mode != FQ_FASTQ_SLOTS_FRESH && fqdev::launch_slot_bases(s)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
        if (fqdev::launch_slot_names(s)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
        fqdev::time_end(3);
        if (fqdev::copy_pinned(fe->h_stat.p + 32 * e, F.d_stat.p, 4 * FQT_N_STAT, 0)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
      }
      // the names of every reference batch's first pair, for the caller's order check
      const int n_sub = (int)((n + B - 1) / B);
      TB.first_names.assign((size_t)n_sub * 2 * (size_t)name_stride, 0);
      std::vector<char> &fn = TB.first_names;
      for (int sb = 0; sb < n_sub; ++sb)
        for (int e = 0; e < NF; ++e)
          if (fqdev::d2h(&fn[((size_t)sb * 2 + e) * name_stride], fe->d_names[slot].p + ((size_t)e * n + (size_t)sb * B) * name_stride, (size_t)name_stride)) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
      if (fqdev::sync()) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
      for (int e = 0; e < NF; ++e) if (fe->h_stat.p[32 * e + FQT_SHORTER_AFTER_LONGER]) fe->f[e].shorter_after_longer = 1;
      TB.d_text[0] = fe->f[0].d_text[slot].p + view[0]; TB.d_text[1] = NF > 1 ? fe->f[1].d_text[slot].p + view[1] : nullptr;
      TB.d_rec = fe->d_rec[slot].p; TB.d_head = fe->d_head[slot].p; TB.d_hlen = fe->d_hlen[slot].p; TB.d_names = fe->d_names[slot].p;
    }
    // ---- what stays for the next chunk: the text behind record n ----
    for (int e = 0; e < NF; ++e) {
      FileSide &F = fe->f[e];
      uint32_t cut = skip[e];
      if (n > 0) {
        if (fqdev::d2h(&cut, F.d_nl.p + 4 * (size_t)n - 1, 4) || fqdev::sync()) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
        cut += 1;
      }
      F.carry_slot = slot; F.carry_off = view[e] + cut; F.carry_len = n_text[e] - cut;
      const int64_t recs = (int64_t)(n_lines[e] / 4);
      if (recs > 0 && n_text[e] > 0) {
        uint32_t last_nl = 0;
        const size_t cap_lines = (size_t)(4 * (fe->chunk_pairs + B));
        const size_t idx = std::min<size_t>((size_t)recs * 4, cap_lines) - 1;
        if (fqdev::d2h(&last_nl, F.d_nl.p + idx, 4) || fqdev::sync()) { finish(FQ_ENODEV, fqdev::last_error(), false); return; }
        F.text_per_record = (double)(last_nl + 1 - skip[e]) / (double)((idx + 1) / 4);
      }
      F.records_done += n;
      {
        std::lock_guard<std::mutex> lk(F.mu);
        F.want_text = (uint64_t)std::min<double>((double)kMaxText, (double)fe->chunk_pairs * F.text_per_record * 1.005 + (256 << 10));
      }
    }
    fe->pairs_done += n;
    fqdev::time_collect(t_ms, t_n, FQ_K_COUNT);
    fe->ms_inflate += t_ms[0]; fe->ms_lines += t_ms[1]; fe->ms_records += t_ms[2]; fe->ms_slots += t_ms[3]; fe->ms_tokenise += t_ms[1] + t_ms[2] + t_ms[3];
    fe->n_launch_inflate += (int64_t)t_n[0]; fe->n_chunks += 1;
    fe->bam.ms_starts += t_ms[4]; fe->bam.ms_pairs += t_ms[5]; fe->bam.ms_fill += t_ms[6]; fe->bam.ms_tags += t_ms[12];
    for (int k = 0; k < 5; ++k) fe->bam.K.ms[k] += t_ms[7 + k];
    fe->n_members += TB.members; fe->n_refused += TB.refused; fe->text_bytes += TB.text_bytes; fe->comp_bytes += TB.comp_bytes;
    {   // how many pairs follow this batch, by the files' sizes and the bytes a pair has taken so far (a hint: fq_align_text sizes a short first call's buffers by it)
      double left = 0;
      for (int e = 0; e < NF; ++e) left += (double)fe->f[e].file_size;
      left -= (double)fe->comp_bytes;
      TB.pairs_behind = fe->comp_bytes > 0 && left > 0 ? (int64_t)(left * (double)fe->pairs_done / (double)fe->comp_bytes) : 0;
    }
    // ---- the end of the stream, or of the device's part of it ----
    bool stream_end = false;
    if (last) {
      // nothing but whole records may be left: otherwise the host's reader says what the rest is (a last record without line end, blank
      // lines, a partner file that goes on)
      bool clean = true;
      for (int e = 0; e < NF; ++e) if (fe->f[e].carry_len != 0) clean = false;
      if (clean) stream_end = true; else fall = true;
    }
    if (!last && !fall && n == 0) {
      // not one whole reference batch yet: the text is carried into the next chunk -- unless a whole chunk's worth of text is there already
      // (reads of many kilobytes): not the device's case
      for (int e = 0; e < NF; ++e) if ((double)n_text[e] >= (double)fe->chunk_pairs * fe->f[e].text_per_record && n_text[e] > ((uint64_t)4 << 20)) fall = true;
    }
    if (stream_end || fall) {
      // (a chunk whose members were started ahead is dropped: the hand-over stands behind this chunk, F.inflated_file_off)
      if (next.open) { if (fe->overlap) { fqdev::stream_aux(1); (void)fqdev::sync(); fqdev::stream_aux(0); } }
      (void)fqdev::sync();
      double t2[FQ_K_COUNT] = {0}; uint64_t n2[FQ_K_COUNT] = {0};
      fqdev::time_collect(t2, n2, FQ_K_COUNT);
      if (stream_end) { fe->ms_inflate += t2[0]; fe->n_launch_inflate += (int64_t)n2[0]; }
    }
    {
      std::lock_guard<std::mutex> lk(fe->mu);
      if (n > 0) fe->ready.push_back(&TB); else fe->slot_free[slot] = true;
      if (fall && fe->bam.on) {          // (no host reader stands behind BAM input: what would hand a FASTQ stream over is an error)
        fe->rc = FQ_ELIMIT; fall = false; stream_end = true;
        fe->err = fe->f[0].path + ": the text of a BAM record is not taken by the tokeniser: a read longer than the rows (" + std::to_string(fe->max_len) + " bases; --read_len), or a name it refuses";
      }
      if (stream_end || fall) { fe->done = true; fe->fallback = fall; if (next.open) fe->slot_free[next.slot] = true; }
      fe->cv.notify_all();
    }
    if (stream_end || fall) return;
  }
}
}  // namespace

fq_frontend::~fq_frontend() {
  { std::lock_guard<std::mutex> lk(mu); stop = true; }
  cv.notify_all();
  for (int e = 0; e < 2; ++e) {
    { std::lock_guard<std::mutex> lk(f[e].mu); f[e].stop = true; }
    f[e].cv.notify_all();
  }
  if (producer.joinable()) producer.join();
  for (int e = 0; e < 2; ++e) {
    if (f[e].th.joinable()) f[e].th.join();
    if (f[e].fd >= 0) close(f[e].fd);
  }
  // (device buffers are freed by the members' destructors; the states last)
  if (st) { fqdev::bind(st); }
}


// fq2 NULL / "": a single-end file (BwtMapper::SingleEndMapper's reader hands out fresh buffers: slot_mode is FRESH whatever is asked).
extern "C" int fq_frontend_open(int device, const char *fq1, const char *fq2, int32_t batch_pairs, int64_t chunk_pairs, int32_t slot_mode, int32_t max_read_len, fq_frontend_t **out) {
  if (!fq1 || !out || batch_pairs < 1 || chunk_pairs < batch_pairs || slot_mode < 0 || slot_mode > 2 || max_read_len < 16 || max_read_len > 4096) return FQ_EINVAL;
  *out = nullptr;
  // (declared in front of `fe`: destroyed behind it -- the device states of an open that fails go when the members' buffers have been freed;
  //  ~fq_frontend leaves them to fq_frontend_close, which an object that was never handed out does not reach)
  struct StatesGuard { fqdev::State *s[3] = {nullptr, nullptr, nullptr}; bool armed = true; ~StatesGuard() { if (armed) for (fqdev::State *x : s) if (x) fqdev::state_destroy(x); } } guard;
  std::unique_ptr<fq_frontend> fe(new fq_frontend);
  fe->device = device; fe->batch_pairs = batch_pairs; fe->chunk_pairs = chunk_pairs / batch_pairs * batch_pairs; fe->max_len = max_read_len;
  fe->n_files = (fq2 && *fq2) ? 2 : 1;
  if (const char *ev = getenv("FASTQUICK_FE_HEADROOM")) fe->headroom_min = strtoull(ev, nullptr, 10);                 // (0: none at all -- the carried text always moves the new text back)
  if (const char *ev = getenv("FASTQUICK_FE_OVERLAP")) fe->overlap = atoi(ev) != 0;      // (0: measurements of the kernels on their own)
  fe->slot_mode = fe->n_files == 1 ? FQ_FASTQ_SLOTS_FRESH : slot_mode;
  const char *paths[2] = {fq1, fq2};
  for (int e = 0; e < fe->n_files; ++e) {
    FileSide &F = fe->f[e];
    F.path = paths[e];
    struct stat sb;
    if (stat(paths[e], &sb) != 0 || !S_ISREG(sb.st_mode)) return FQ_EIO;           // (a pipe cannot be looked at twice: the host reader's case)
    F.fd = open(paths[e], O_RDONLY);
    if (F.fd < 0) return FQ_EIO;
    uint8_t h[1 << 16];
    const ssize_t got = pread(F.fd, h, sizeof h, 0);
    size_t hdr = 0;
    const size_t sz = got >= 18 ? bgzf_member(h, (size_t)got, &hdr) : 0;
    if (sz == 0) return FQ_EIO;
    F.file_size = (uint64_t)sb.st_size;
    if (sz >= hdr + 8 && (size_t)got >= sz && le32(h + sz - 4)) F.comp_ratio = (double)sz / (double)le32(h + sz - 4);                                                     // not BGZF: the host reader's case
    // the text a record takes, from the file's first member (inflated here, on the host: 64 KiB)
    F.text_per_record = 320.0;
    if ((size_t)got >= sz && sz >= hdr + 8) {
      const uint32_t isize = le32(h + sz - 4);
      std::vector<uint8_t> t(isize + 1);
      std::unique_ptr<fqz::Inflater> fz(new fqz::Inflater);
      if (isize && fqz::inflate_raw(*fz, h + hdr, sz - hdr - 8, t.data(), isize)) {
        size_t lines = 0, last = 0;
        for (size_t i = 0; i < isize; ++i) if (t[i] == '\n') { ++lines; if (lines % 4 == 0) last = i + 1; }
        if (lines >= 4) F.text_per_record = (double)last / (double)(lines / 4);
      }
    }
  }
  // device side
  fe->st = guard.s[0] = fqdev::state_create(device);
  if (!fe->st || fqdev::bind(fe->st)) return FQ_ENODEV;
  const size_t n_slots = (size_t)2 * (size_t)batch_pairs;
  for (int e = 0; e < fe->n_files; ++e) {
    FileSide &F = fe->f[e];
    F.st = guard.s[1 + e] = fqdev::state_create(device);
    if (!F.st) return FQ_ENODEV;
    if (fqdev::bind(fe->st)) return FQ_ENODEV;
    if (!F.d_slot_base.ensure(n_slots * 96) || !F.d_slot_len.ensure(n_slots) || !F.d_slot_name.ensure(n_slots * 304) || !F.d_stat.ensure(FQT_N_STAT + 8)) return FQ_ENOMEM;
    if (fqdev::dzero(F.d_slot_base.p, n_slots * 96) || fqdev::dzero(F.d_slot_len.p, n_slots * 2) || fqdev::dzero(F.d_slot_name.p, n_slots * 304)) return FQ_ENODEV;
  }
  if (fqdev::sync()) return FQ_ENODEV;
  for (int e = 0; e < fe->n_files; ++e) {
    fe->f[e].want_text = (uint64_t)std::min<double>((double)kMaxText, (double)fe->chunk_pairs * fe->f[e].text_per_record * 1.005 + (256 << 10));
    fe->f[e].read_threads = std::max(1, std::min(4, fq_host_cpus() / (2 * fe->n_files)));     // (of the CPUs this process may use: fq_host_cpus)
    if (const char *ev = getenv("FASTQUICK_FE_READ_THREADS")) fe->f[e].read_threads = std::max(1, std::min(16, atoi(ev)));
    fe->f[e].th = std::thread(reader_main, fe.get(), e);
  }
  fe->producer = std::thread(producer_main, fe.get());
  guard.armed = false;
  *out = fe.release();
  return FQ_OK;
}
// ---- BAM input: the host's look at the file (header, first kept record), and the open ---------------------------------------------------
namespace {
// the payload of a BGZF file member by member, through zlib: only for the header and the first records (fq_bam_probe)
struct HostBgzf {
  int fd = -1;
  int64_t at = 0, cur_off = 0;                 // file offset of the next member; of the member `cur` came from
  std::vector<uint8_t> cur;
  size_t pos = 0;
  bool not_bgzf = false, corrupt = false;
  bool fill() {                                // the next member that holds payload; false at the end of the file or on an error
    for (;;) {
      uint8_t h[18 + 256];
      const ssize_t got = pread(fd, h, sizeof h, (off_t)at);
      if (got <= 0) return false;
      size_t hdr = 0;
      const size_t sz = got >= 18 ? bgzf_member(h, (size_t)got, &hdr) : 0;
      if (sz == 0 || sz < hdr + 8) { not_bgzf = true; return false; }
      std::vector<uint8_t> m(sz);
      if (pread(fd, m.data(), sz, (off_t)at) != (ssize_t)sz) { corrupt = true; return false; }
      const uint32_t isize = le32(m.data() + sz - 4);
      cur_off = at; at += (int64_t)sz;
      if (isize == 0) continue;
      cur.assign(isize, 0); pos = 0;
      z_stream zs;
      memset(&zs, 0, sizeof zs);
      if (inflateInit2(&zs, -15) != Z_OK) { corrupt = true; return false; }
      zs.next_in = m.data() + hdr; zs.avail_in = (uInt)(sz - hdr - 8); zs.next_out = cur.data(); zs.avail_out = isize;
      const int zr = inflate(&zs, Z_FINISH);
      const bool ok = zr == Z_STREAM_END && zs.avail_out == 0;
      inflateEnd(&zs);
      if (!ok) { corrupt = true; return false; }
      return true;
    }
  }
  bool read(uint8_t *dst, size_t n) {          // false: the stream ends (or fails) inside these n bytes
    while (n) {
      if (pos == cur.size() && !fill()) return false;
      const size_t take = std::min(n, cur.size() - pos);
      if (dst) { memcpy(dst, cur.data() + pos, take); dst += take; }
      pos += take; n -= take;
    }
    return true;
  }
};
}  // namespace

// The host's look at a BAM file: BGZF, magic, the header (it may span several members), where the records begin, and the first record that is
// kept (neither secondary nor supplementary) -- its flag says paired or single-end, its l_seq sizes the rows.  Stands in for the open of the
// reference's dormant bwa_read_bam (libbwa/bwaseqio.c:90-142).  FQ_OK, or FQ_EIO with out->error.
static int probe_bam(const char *path, const fq_bam_select_t *sel, fq_bam_probe_t *out, std::string *header_text) {
  if (!path || !out) return FQ_EINVAL;
  std::vector<uint32_t> ids;                     // (--bam_rg: "kept" is then what the tag body says, on the whole record)
  pack_bam_ids(sel, &ids);
  std::vector<uint8_t> rec;
  memset(out, 0, sizeof *out);
  out->first_flag = -1;
  auto fail = [&](const std::string &m) { snprintf(out->error, sizeof out->error, "%s: %s", path, m.c_str()); return FQ_EIO; };
  HostBgzf z;
  struct stat sb;
  if (stat(path, &sb) != 0 || !S_ISREG(sb.st_mode)) return fail("not a regular file");
  z.fd = open(path, O_RDONLY);
  if (z.fd < 0) return fail("cannot be opened");
  struct Closer { int fd; ~Closer() { close(fd); } } closer{z.fd};
  static const uint8_t eof_block[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint8_t tail[28];
  out->has_eof_block = sb.st_size >= 28 && pread(z.fd, tail, 28, (off_t)sb.st_size - 28) == 28 && memcmp(tail, eof_block, 28) == 0;
  auto why = [&](const char *where) { return z.not_bgzf ? std::string("not a BGZF file (a BAM file is BGZF: gzip members with a BC field)") : z.corrupt ? std::string("corrupt BGZF member") : std::string("the stream ends inside ") + where; };
  uint8_t w[8];
  if (!z.read(w, 4)) return fail(why("the header"));
  if (memcmp(w, "BAM\1", 4) != 0) return fail("no BAM magic at the start of the stream");
  if (!z.read(w, 4)) return fail(why("the header"));
  const uint32_t l_text = le32(w);
  if ((uint64_t)l_text > (uint64_t)sb.st_size * 1100 + 65536) return fail("the header's text length is not one this file can hold");      // (DEFLATE expands by 1032 at most)
  std::vector<uint8_t> text(l_text);
  if (l_text && !z.read(text.data(), l_text)) return fail(why("the header"));
  if (header_text) header_text->assign((const char *)text.data(), text.size());
  {   // @HD ... SO:value
    const std::string t((const char *)text.data(), text.size());
    if (t.compare(0, 3, "@HD") == 0) {
      const size_t eol = t.find('\n'), so = t.find("\tSO:");
      if (so != std::string::npos && (eol == std::string::npos || so < eol)) {
        size_t e = so + 4;
        while (e < t.size() && t[e] != '\t' && t[e] != '\n' && e - so - 4 < sizeof out->sort_order - 1) ++e;
        memcpy(out->sort_order, t.data() + so + 4, e - so - 4);
      }
    }
  }
  if (!z.read(w, 4)) return fail(why("the header"));
  const uint32_t n_ref = le32(w);
  if (n_ref > 0x7fffffffu) return fail("the header's reference count is not one");
  for (uint32_t r = 0; r < n_ref; ++r) {
    if (!z.read(w, 4)) return fail(why("the header"));
    const uint32_t l_name = le32(w);
    if (l_name > (1u << 20) || !z.read(nullptr, (size_t)l_name + 4)) return fail(why("the header"));
    out->header_bytes += 8 + (int64_t)l_name;
  }
  out->n_ref = (int32_t)n_ref;
  out->header_bytes += 12 + (int64_t)l_text;
  if (z.pos == z.cur.size()) { out->rec_member_off = z.at; out->rec_off = 0; } else { out->rec_member_off = z.cur_off; out->rec_off = (int64_t)z.pos; }
  // the first kept record
  for (;;) {
    uint8_t fx[36];
    if (!z.read(fx, 4)) break;                  // (no record, or the end: the stream's own walk says what is wrong, if anything)
    const uint32_t bs = le32(fx);
    if (bs < 32 || bs > FQB_MAX_BLOCK || !z.read(fx + 4, 32)) break;
    const uint32_t flag = fx[18] | (uint32_t)fx[19] << 8;
    bool kept = !(flag & 0x900u), whole = false;
    if (kept && !ids.empty()) {
      rec.resize((size_t)bs + 4);
      memcpy(rec.data(), fx, 36);
      if (!z.read(rec.data() + 36, bs - 32)) break;
      whole = true;
      uint32_t k = 0, oq = 0, unsel = 0;
      (void)fq_bam_tags_record(rec.data(), ids.data(), 0, &k, &oq, &unsel);      // (a walk that fails: the stream's own walk refuses the record)
      kept = k != 0;
    }
    if (kept) {
      const int32_t l = (int32_t)std::min<uint32_t>(le32(fx + 20), 0x7fffffffu);
      if (out->first_flag >= 0) { out->first_l_seq = std::max(out->first_l_seq, l); break; }      // (the second kept record of a paired stream: the rows hold the first pair's longer read, as the FASTQ path's do)
      out->first_flag = (int32_t)flag; out->paired = (int32_t)(flag & 1u); out->first_l_seq = l; out->first_l_name = fx[12];
      if (!out->paired) break;
    }
    if (!whole && !z.read(nullptr, bs - 32)) break;
  }
  return FQ_OK;
}
extern "C" int fq_bam_probe(const char *path, fq_bam_probe_t *out) { return probe_bam(path, nullptr, out, nullptr); }
extern "C" int fq_bam_probe_select(const char *path, const fq_bam_select_t *sel, fq_bam_probe_t *out) { return probe_bam(path, sel, out, nullptr); }
// The ID values of the header's @RG lines, in the header's order, each with its NUL, one behind the other in ids[cap]; *n_ids of them take *bytes
// (FQ_ELIMIT where cap is smaller: call again).  FQ_EIO as fq_bam_probe, which this runs.
extern "C" int fq_bam_read_groups(const char *path, char *ids, int64_t cap, int32_t *n_ids, int64_t *bytes) {
  if (!path || !n_ids || !bytes || cap < 0 || (cap && !ids)) return FQ_EINVAL;
  fq_bam_probe_t pr;
  std::string text, all;
  *n_ids = 0; *bytes = 0;
  if (const int rc = probe_bam(path, nullptr, &pr, &text)) return rc;
  for (size_t at = 0; at < text.size();) {
    size_t eol = text.find('\n', at);
    if (eol == std::string::npos) eol = text.size();
    if (text.compare(at, 4, "@RG\t") == 0) {
      for (size_t f = at + 3; f < eol;) {          // (f: at a tab)
        size_t g = text.find('\t', f + 1);
        if (g == std::string::npos || g > eol) g = eol;
        if (text.compare(f + 1, 3, "ID:") == 0) { all.append(text, f + 4, g - f - 4); all.push_back('\0'); ++*n_ids; break; }
        f = g;
      }
    }
    at = eol + 1;
  }
  *bytes = (int64_t)all.size();
  if ((int64_t)all.size() > cap) return FQ_ELIMIT;
  if (!all.empty()) memcpy(ids, all.data(), all.size());
  return FQ_OK;
}

// One BAM file -> the batches fq_frontend_open gives for the two FASTQ texts its records transcode to (include/fastquick_amd.h).
// collate_mem < 0: mates are adjacent (fq_frontend_open_bam); otherwise they are found by name, and the records waiting for theirs take so many bytes at most.
static int open_bam(int device, const char *bam, int32_t batch_pairs, int64_t chunk_pairs, int32_t slot_mode, int32_t max_read_len, int64_t collate_mem, const fq_bam_select_t *sel, fq_frontend_t **out) {
  if (!bam || !out || batch_pairs < 1 || chunk_pairs < batch_pairs || slot_mode < 0 || slot_mode > 2 || max_read_len < 16 || max_read_len > 4096) return FQ_EINVAL;
  *out = nullptr;
  fq_bam_probe_t pr;
  if (sel && (sel->n_ids < 0 || (sel->n_ids && !sel->ids))) return FQ_EINVAL;
  if (const int rc = probe_bam(bam, sel, &pr, nullptr)) return rc;
  if (!pr.has_eof_block) fprintf(stderr, "WARNING - %s: no BGZF end-of-file block at the end of the file: it may be truncated\n", bam);
  struct StatesGuard { fqdev::State *s[3] = {nullptr, nullptr, nullptr}; bool armed = true; ~StatesGuard() { if (armed) for (fqdev::State *x : s) if (x) fqdev::state_destroy(x); } } guard;
  std::unique_ptr<fq_frontend> fe(new fq_frontend);
  fe->device = device; fe->batch_pairs = batch_pairs; fe->chunk_pairs = chunk_pairs / batch_pairs * batch_pairs; fe->max_len = max_read_len;
  fe->n_files = pr.paired ? 2 : 1;
  if (const char *ev = getenv("FASTQUICK_FE_HEADROOM")) fe->headroom_min = strtoull(ev, nullptr, 10);
  fe->overlap = false;                           // (BAM chunks run one after the other: bam_chunk)
  fe->slot_mode = fe->n_files == 1 ? FQ_FASTQ_SLOTS_FRESH : slot_mode;
  fe->bam.on = true; fe->bam.n_ref = pr.n_ref; fe->bam.paired = pr.paired; fe->bam.first_off = (uint64_t)pr.rec_off;
  fe->bam.K.on = collate_mem >= 0; fe->bam.K.mem = collate_mem >= 0 ? (uint64_t)collate_mem : 0;
  fe->bam.W.select(sel);
  const double l_name = pr.first_flag >= 0 ? (double)pr.first_l_name : 20.0, l_seq = pr.first_flag >= 0 ? (double)pr.first_l_seq : 151.0;
  for (int e = 0; e < fe->n_files; ++e) {
    FileSide &F = fe->f[e];
    F.path = bam;
    F.text_per_record = l_name + 2.0 * l_seq + 5.0;
    F.all_launched = e > 0;                      // (one compressed side: the second text has no reader of its own)
  }
  {
    FileSide &F = fe->f[0];
    struct stat sb;
    if (stat(bam, &sb) != 0) return FQ_EIO;
    F.fd = open(bam, O_RDONLY);
    if (F.fd < 0) return FQ_EIO;
    F.file_size = (uint64_t)sb.st_size;
    F.file_off = pr.rec_member_off;
    F.want_scale = (double)fe->n_files * (36.0 + l_name + 1.5 * l_seq) / F.text_per_record;
  }
  fe->st = guard.s[0] = fqdev::state_create(device);
  if (!fe->st || fqdev::bind(fe->st)) return FQ_ENODEV;
  fe->f[0].st = guard.s[1] = fqdev::state_create(device);
  if (!fe->f[0].st || fqdev::bind(fe->st)) return FQ_ENODEV;
  const size_t n_slots = (size_t)2 * (size_t)batch_pairs;
  for (int e = 0; e < fe->n_files; ++e) {
    FileSide &F = fe->f[e];
    if (!F.d_slot_base.ensure(n_slots * 96) || !F.d_slot_len.ensure(n_slots) || !F.d_slot_name.ensure(n_slots * 304) || !F.d_stat.ensure(FQT_N_STAT + 8)) return FQ_ENOMEM;
    if (fqdev::dzero(F.d_slot_base.p, n_slots * 96) || fqdev::dzero(F.d_slot_len.p, n_slots * 2) || fqdev::dzero(F.d_slot_name.p, n_slots * 304)) return FQ_ENODEV;
    F.want_text = (uint64_t)std::min<double>((double)kMaxText, (double)fe->chunk_pairs * F.text_per_record * 1.005 + (256 << 10));
  }
  if (fqdev::sync()) return FQ_ENODEV;
  fe->f[0].read_threads = std::max(1, std::min(4, fq_host_cpus() / 2));
  if (const char *ev = getenv("FASTQUICK_FE_READ_THREADS")) fe->f[0].read_threads = std::max(1, std::min(16, atoi(ev)));
  fe->f[0].th = std::thread(reader_main, fe.get(), 0);
  fe->producer = std::thread(producer_main, fe.get());
  guard.armed = false;
  *out = fe.release();
  return FQ_OK;
}
extern "C" int fq_frontend_open_bam(int device, const char *bam, int32_t batch_pairs, int64_t chunk_pairs, int32_t slot_mode, int32_t max_read_len, fq_frontend_t **out) {
  return open_bam(device, bam, batch_pairs, chunk_pairs, slot_mode, max_read_len, -1, nullptr, out);
}
extern "C" int fq_frontend_open_bam_select(int device, const char *bam, int32_t batch_pairs, int64_t chunk_pairs, int32_t slot_mode, int32_t max_read_len, const fq_bam_select_t *sel, fq_frontend_t **out) {
  return open_bam(device, bam, batch_pairs, chunk_pairs, slot_mode, max_read_len, -1, sel, out);
}
extern "C" int fq_frontend_open_bam_collate_select(int device, const char *bam, int32_t batch_pairs, int64_t chunk_pairs, int32_t slot_mode, int32_t max_read_len, int64_t collate_mem_bytes, const fq_bam_select_t *sel,
                                                   fq_frontend_t **out) {
  if (collate_mem_bytes < 0) return FQ_EINVAL;
  return open_bam(device, bam, batch_pairs, chunk_pairs, slot_mode, max_read_len, collate_mem_bytes, sel, out);
}
extern "C" int fq_frontend_open_bam_collate(int device, const char *bam, int32_t batch_pairs, int64_t chunk_pairs, int32_t slot_mode, int32_t max_read_len, int64_t collate_mem_bytes, fq_frontend_t **out) {
  if (collate_mem_bytes < 0) return FQ_EINVAL;
  return open_bam(device, bam, batch_pairs, chunk_pairs, slot_mode, max_read_len, collate_mem_bytes, nullptr, out);
}

// Kernels (a)-(c) on their own (tests, measurement): a payload in host memory, cut into members where the caller says.
static int bam_transcode_device(int device, const uint8_t *payload, size_t n, const int64_t *member_off, int64_t n_members, int32_t n_ref, int64_t first_record, int32_t paired,
                                uint8_t *text1, size_t cap1, uint8_t *text2, size_t cap2, uint32_t *starts, int64_t starts_cap, const fq_bam_select_t *sel, fq_bam_tag_counts_t *counts, fq_bam_transcode_t *out) {
  if (counts) memset(counts, 0, sizeof *counts);
  if (sel && (sel->n_ids < 0 || (sel->n_ids && !sel->ids))) return FQ_EINVAL;
  if (!out || (n && !payload) || n > 0xfff00000ull || first_record < 0 || (uint64_t)first_record > n || n_members < 0 || (n_members && !member_off)) return FQ_EINVAL;
  memset(out, 0, sizeof *out);
  DevScope scope(device);
  if (!scope.s || fqdev::bind(scope.s)) return FQ_ENODEV;
  int rc = FQ_OK;
  {
    BamWork W;
    W.select(sel);
    // (payload and texts are allocated to the byte: under the host-loop build a kernel body that reads behind the payload or writes behind a text is a sanitizer's finding)
    DevMem d_pay, d_text[2];
    if (!d_pay.alloc(std::max<size_t>(n, 1))) return FQ_ENOMEM;
    if ((n && fqdev::h2d(d_pay.p, payload, n)) || fqdev::sync()) return FQ_ENODEV;
    std::vector<uint32_t> cuts;
    for (int64_t k = 0; k < n_members; ++k) {
      if (member_off[k] < 0 || (uint64_t)member_off[k] > n || (k && member_off[k] < member_off[k - 1])) return FQ_EINVAL;
      cuts.push_back((uint32_t)member_off[k]);
    }
    BamChunk R;
    std::string err;
    rc = bam_records(W, (const uint8_t *)d_pay.p, (uint32_t)n, (uint32_t)first_record, cuts, n_ref, paired, 0, &R, &err);
    if (rc) return rc;
    out->records = R.n_rec; out->kept = R.n_kept; out->units = R.n_units; out->used_records = R.used_rec; out->paired = R.paired; out->chain_repairs = R.repairs;
    out->text_len[0] = (int64_t)R.text_len[0]; out->text_len[1] = (int64_t)R.text_len[1]; out->chain_end = R.chain_end; out->carry_from = R.carry_from; out->end_flag = R.end_flag;
    out->bad_record = R.bad == FQB_NO_BAD ? -1 : (int64_t)fqb_bad_ord(R.bad); out->bad_kind = R.bad == FQB_NO_BAD ? 0 : (int32_t)fqb_bad_kind(R.bad);
    if (counts) { counts->unselected = R.n_unsel; counts->oq_records = R.n_oq; }
    if (starts && R.n_rec) {
      if ((int64_t)R.n_rec > starts_cap) return FQ_ELIMIT;
      if (fqdev::d2h(starts, W.starts.p, 4 * (size_t)R.n_rec) || fqdev::sync()) return FQ_ENODEV;
    }
    if (R.bad == FQB_NO_BAD) {
      if (R.text_len[0] > cap1 || R.text_len[1] > cap2) return FQ_ELIMIT;
      uint8_t *text[2] = {nullptr, nullptr};
      uint8_t *host[2] = {text1, text2};
      for (int e = 0; e < (R.paired ? 2 : 1); ++e) { if (!d_text[e].alloc((size_t)R.text_len[e] + 3 * e + 1)) return FQ_ENOMEM; text[e] = (uint8_t *)d_text[e].p + 3 * e; }      // (the second text begins off a dword)
      if ((rc = bam_fill(W, (const uint8_t *)d_pay.p, R, text, &err))) return rc;
      for (int e = 0; e < (R.paired ? 2 : 1); ++e) if (R.text_len[e] && (!host[e] || fqdev::d2h(host[e], text[e], (size_t)R.text_len[e]))) return FQ_ENODEV;
      if (fqdev::sync()) return FQ_ENODEV;
    }
    double ms[FQ_K_COUNT] = {0};
    uint64_t ln[FQ_K_COUNT] = {0};
    fqdev::time_collect(ms, ln, FQ_K_COUNT);
    out->ms_starts = ms[4]; out->ms_pairs = ms[5]; out->ms_fill = ms[6];
    if (counts) counts->ms_tags = ms[12];
  }
  return rc;
}
extern "C" int fq_bam_transcode_device(int device, const uint8_t *payload, size_t n, const int64_t *member_off, int64_t n_members, int32_t n_ref, int64_t first_record, int32_t paired,
                                       uint8_t *text1, size_t cap1, uint8_t *text2, size_t cap2, uint32_t *starts, int64_t starts_cap, fq_bam_transcode_t *out) {
  return bam_transcode_device(device, payload, n, member_off, n_members, n_ref, first_record, paired, text1, cap1, text2, cap2, starts, starts_cap, nullptr, nullptr, out);
}
extern "C" int fq_bam_transcode_device_select(int device, const uint8_t *payload, size_t n, const int64_t *member_off, int64_t n_members, int32_t n_ref, int64_t first_record, int32_t paired,
                                              uint8_t *text1, size_t cap1, uint8_t *text2, size_t cap2, uint32_t *starts, int64_t starts_cap, const fq_bam_select_t *sel, fq_bam_tag_counts_t *counts,
                                              fq_bam_transcode_t *out) {
  return bam_transcode_device(device, payload, n, member_off, n_members, n_ref, first_record, paired, text1, cap1, text2, cap2, starts, starts_cap, sel, counts, out);
}
// The collating chunk loop on its own (tests, measurement): the payload is taken up in chunks of members_per_chunk members each, as the front end
// takes up a stream -- the record a chunk's end cuts off leads the next chunk's payload, the records waiting for their mates are held in HBM --, and
// both texts are written chunk after chunk.
static int bam_collate_device(int device, const uint8_t *payload, size_t n, const int64_t *member_off, int64_t n_members, int64_t members_per_chunk, int32_t n_ref, int64_t first_record,
                              int32_t paired, int64_t collate_mem_bytes, uint8_t *text1, size_t cap1, uint8_t *text2, size_t cap2, const fq_bam_select_t *sel, fq_bam_tag_counts_t *counts, fq_bam_collate_t *out) {
  if (counts) memset(counts, 0, sizeof *counts);
  if (sel && (sel->n_ids < 0 || (sel->n_ids && !sel->ids))) return FQ_EINVAL;
  std::vector<uint32_t> ids;
  pack_bam_ids(sel, &ids);
  if (!out || (n && !payload) || n > 0xfff00000ull || first_record < 0 || (uint64_t)first_record > n || n_members < 0 || (n_members && !member_off) || collate_mem_bytes < 0 || paired < -1 || paired > 1) return FQ_EINVAL;
  memset(out, 0, sizeof *out);
  out->bad_record = -1;
  for (int64_t k = 0; k < n_members; ++k) if (member_off[k] < 0 || (uint64_t)member_off[k] > n || (k && member_off[k] < member_off[k - 1])) return FQ_EINVAL;
  if (paired < 0) {      // by the first kept record (the front end knows it from fq_bam_probe)
    paired = 0;
    for (uint64_t p = (uint64_t)first_record; p + 36 <= n;) {
      const uint32_t bs = le32(payload + p), flag = payload[p + 18] | (uint32_t)payload[p + 19] << 8;
      if (bs < 32 || bs > FQB_MAX_BLOCK) break;
      bool kept = !(flag & 0x900u);
      if (kept && !ids.empty()) {                 // (under a selection, as the probe: the tag body on the whole record)
        if (p + 4 + (uint64_t)bs > n) break;
        uint32_t k = 0, oq = 0, unsel = 0;
        (void)fq_bam_tags_record(payload + p, ids.data(), 0, &k, &oq, &unsel);
        kept = k != 0;
      }
      if (kept) { paired = (int32_t)(flag & 1u); break; }
      p += 4 + (uint64_t)bs;
    }
  }
  out->paired = paired;
  DevScope scope(device);
  if (!scope.s || fqdev::bind(scope.s)) return FQ_ENODEV;
  const int64_t per = members_per_chunk > 0 ? members_per_chunk : std::max<int64_t>(n_members, 1);
  const int64_t n_chunks = std::max<int64_t>(1, (n_members + per - 1) / per);
  BamWork W;
  BamHeld K;
  K.on = true; K.mem = (uint64_t)collate_mem_bytes;
  W.select(sel);
  std::vector<uint8_t> carry;                    // the record the last chunk's end cut off
  uint64_t ord0 = 0, text_at[2] = {0, 0};
  uint8_t *host[2] = {text1, text2};
  const size_t cap[2] = {cap1, cap2};
  std::string err;
  int rc = FQ_OK;
  auto fail = [&](int code) { snprintf(out->error, sizeof out->error, "%s", err.c_str()); return code; };
  for (int64_t j = 0; j < n_chunks && rc == FQ_OK; ++j) {
    const uint64_t lo = j == 0 ? 0 : (uint64_t)member_off[j * per], hi = j + 1 == n_chunks ? n : (uint64_t)member_off[(j + 1) * per];
    const bool last = j + 1 == n_chunks;
    if (!carry.size() && (uint64_t)first_record >= hi && !last) continue;      // (the header's chunks)
    const uint64_t cl = carry.size(), m = cl + (hi - lo);
    // (payload and texts are allocated to the byte, as in fq_bam_transcode_device)
    DevMem d_pay, d_text[2];
    if (!d_pay.alloc(std::max<size_t>((size_t)m, 1))) return FQ_ENOMEM;
    if ((cl && fqdev::h2d(d_pay.p, carry.data(), (size_t)cl)) || (hi > lo && fqdev::h2d((uint8_t *)d_pay.p + cl, payload + lo, (size_t)(hi - lo))) || fqdev::sync()) return FQ_ENODEV;
    const uint32_t rec0 = cl ? 0u : (uint32_t)((uint64_t)first_record > lo ? (uint64_t)first_record - lo : 0);
    std::vector<uint32_t> cuts;
    for (int64_t k = j * per; k < std::min<int64_t>(n_members, (j + 1) * per); ++k) if ((uint64_t)member_off[k] >= lo) cuts.push_back((uint32_t)((uint64_t)member_off[k] - lo + cl));
    BamChunk R;
    const bool collate = paired != 0;
    rc = collate ? bam_collate_records(W, K, (const uint8_t *)d_pay.p, (uint32_t)m, rec0, cuts, n_ref, ord0, &R, &err) : bam_records(W, (const uint8_t *)d_pay.p, (uint32_t)m, rec0, cuts, n_ref, 0, ord0, &R, &err);
    if (rc) return fail(rc);
    out->chunks += 1; out->records += R.n_rec; out->kept += R.n_kept; out->pairs += R.n_units; out->end_flag = R.end_flag;
    out->chain_end = (int64_t)(lo + R.chain_end - cl);
    if (counts) { counts->unselected += R.n_unsel; counts->oq_records += R.n_oq; }
    if (R.bad != FQB_NO_BAD) { out->bad_record = (int64_t)fqb_bad_ord(R.bad); out->bad_kind = (int32_t)fqb_bad_kind(R.bad); break; }
    if (R.end_flag == FQB_SEG_CORRUPT) break;
    uint8_t *text[2] = {nullptr, nullptr};
    const int sides = R.paired ? 2 : 1;
    for (int e = 0; e < sides; ++e) {
      if (text_at[e] + R.text_len[e] > cap[e]) { err = "a text does not fit its buffer"; return fail(FQ_ELIMIT); }
      if (!d_text[e].alloc((size_t)R.text_len[e] + 3 * e + 1)) return FQ_ENOMEM;
      text[e] = (uint8_t *)d_text[e].p + 3 * e;      // (the second text begins off a dword)
    }
    if ((rc = bam_fill(W, (const uint8_t *)d_pay.p, R, text, &err, collate ? &K : nullptr))) return fail(rc);
    for (int e = 0; e < sides; ++e) {
      if (R.text_len[e] && (!host[e] || fqdev::d2h(host[e] + text_at[e], text[e], (size_t)R.text_len[e]))) return FQ_ENODEV;
      text_at[e] += R.text_len[e];
    }
    if (fqdev::sync()) return FQ_ENODEV;
    if (collate && (rc = bam_collate_hold(W, K, (const uint8_t *)d_pay.p, ord0, &err))) return fail(rc);
    ord0 += R.n_rec;
    carry.assign((size_t)(m - R.chain_end), 0);
    if (!carry.empty() && (fqdev::d2h(carry.data(), (const uint8_t *)d_pay.p + R.chain_end, carry.size()) || fqdev::sync())) return FQ_ENODEV;
    double ms[FQ_K_COUNT] = {0};
    uint64_t ln[FQ_K_COUNT] = {0};
    fqdev::time_collect(ms, ln, FQ_K_COUNT);
    out->ms_keys += ms[7]; out->ms_sort += ms[8]; out->ms_match += ms[9]; out->ms_units += ms[10]; out->ms_hold += ms[11];
    if (counts) counts->ms_tags += ms[12];
  }
  if (counts && K.n && W.tags && W.use_oq && out->bad_record < 0) {      // (the orphans' OQ values were read by nobody)
    std::vector<uint32_t> hoq(K.n);
    if (fqdev::d2h(hoq.data(), K.oq[K.cur].p, 4 * (size_t)K.n) || fqdev::sync()) return FQ_ENODEV;
    for (uint32_t v : hoq) if (v) --counts->oq_records;
  }
  out->text_len[0] = (int64_t)text_at[0]; out->text_len[1] = (int64_t)text_at[1];
  out->orphans = K.n; out->held_peak_records = K.peak_n; out->held_peak_bytes = K.peak_bytes;
  out->ms_collate = out->ms_keys + out->ms_sort + out->ms_match + out->ms_units + out->ms_hold;
  return FQ_OK;
}
extern "C" int fq_bam_collate_device(int device, const uint8_t *payload, size_t n, const int64_t *member_off, int64_t n_members, int64_t members_per_chunk, int32_t n_ref, int64_t first_record,
                                     int32_t paired, int64_t collate_mem_bytes, uint8_t *text1, size_t cap1, uint8_t *text2, size_t cap2, fq_bam_collate_t *out) {
  return bam_collate_device(device, payload, n, member_off, n_members, members_per_chunk, n_ref, first_record, paired, collate_mem_bytes, text1, cap1, text2, cap2, nullptr, nullptr, out);
}
extern "C" int fq_bam_collate_device_select(int device, const uint8_t *payload, size_t n, const int64_t *member_off, int64_t n_members, int64_t members_per_chunk, int32_t n_ref, int64_t first_record,
                                            int32_t paired, int64_t collate_mem_bytes, uint8_t *text1, size_t cap1, uint8_t *text2, size_t cap2, const fq_bam_select_t *sel, fq_bam_tag_counts_t *counts,
                                            fq_bam_collate_t *out) {
  return bam_collate_device(device, payload, n, member_off, n_members, members_per_chunk, n_ref, first_record, paired, collate_mem_bytes, text1, cap1, text2, cap2, sel, counts, out);
}
extern "C" void fq_frontend_close(fq_frontend_t *fe) {
  if (!fe) return;
  fqdev::State *states[3] = {fe->st, fe->f[0].st, fe->f[1].st};
  const int device = fe->device;
  (void)device;
  delete fe;            // joins the threads, frees the buffers
  for (fqdev::State *s : states) if (s) fqdev::state_destroy(s);
}
extern "C" const char *fq_frontend_last_error(const fq_frontend_t *fe) { return fe ? fe->err.c_str() : ""; }
// The next batch (*out; it stays valid until fq_frontend_release).  Returns its number of pairs; 0 at the end of the stream; FQ_EFALLBACK when
// the rest of the stream is the host reader's (fq_frontend_handover); another negative code on failure (fq_frontend_last_error).
extern "C" int64_t fq_frontend_next(fq_frontend_t *fe, fq_text_batch_t **out) {
  if (!fe || !out) return FQ_EINVAL;
  *out = nullptr;
  std::unique_lock<std::mutex> lk(fe->mu);
  fe->cv.wait(lk, [&] { return !fe->ready.empty() || fe->done; });
  if (!fe->ready.empty()) {
    fq_text_batch *b = fe->ready.front();
    fe->ready.pop_front();
    *out = b;
    return b->n_pairs;
  }
  if (fe->rc) return fe->rc;
  return fe->fallback ? FQ_EFALLBACK : 0;
}
extern "C" void fq_frontend_release(fq_frontend_t *fe, fq_text_batch_t *b) {
  if (!fe || !b || b->slot < 0) return;
  { std::lock_guard<std::mutex> lk(fe->mu); fe->slot_free[b->slot] = true; }
  fe->cv.notify_all();
}
// Host readers standing where the device's part of the stream ended (after fq_frontend_next returned FQ_EFALLBACK and every batch has been
// released): out[e] for each file, opened with `threads` threads each.
extern "C" int fq_frontend_handover(fq_frontend_t *fe, int threads, fq_fastq_t **out) {
  if (!fe || !out) return FQ_EINVAL;
  if (fe->bam.on) return FQ_EINVAL;       // (BAM input: there is no host reader to hand to)
  { std::lock_guard<std::mutex> lk(fe->mu); if (!fe->done || !fe->fallback) return FQ_EINVAL; }
  if (fe->producer.joinable()) fe->producer.join();
  if (fqdev::bind(fe->st)) return FQ_ENODEV;
  const size_t n_slots = (size_t)2 * (size_t)fe->batch_pairs;
  for (int e = 0; e < fe->n_files; ++e) {
    FileSide &F = fe->f[e];
    { std::lock_guard<std::mutex> lk(F.mu); F.stop = true; }
    F.cv.notify_all();
    if (F.th.joinable()) F.th.join();
    const int64_t file_off = F.inflated_file_off;          // behind the last chunk that was inflated (a chunk the reader thread filled ahead has not been used)
    std::vector<uint8_t> text((size_t)F.carry_len), names, bases;
    std::vector<uint16_t> lens;
    if (F.carry_len && fqdev::d2h(text.data(), F.d_text[F.carry_slot].p + F.carry_off, (size_t)F.carry_len)) return FQ_ENODEV;
    if (fe->slot_mode != FQ_FASTQ_SLOTS_FRESH) {
      names.resize(n_slots * 304); bases.resize(n_slots * 96); lens.resize(n_slots);
      if (fqdev::d2h(names.data(), F.d_slot_name.p, names.size()) || fqdev::d2h(bases.data(), F.d_slot_base.p, bases.size()) || fqdev::d2h(lens.data(), F.d_slot_len.p, lens.size() * 2)) return FQ_ENODEV;
    }
    if (fqdev::sync()) return FQ_ENODEV;
    fq_fastq_t *r = nullptr;
    int rc = fq_fastq_open(F.path.c_str(), threads, &r);
    if (rc) return rc;
    fq_fastq_configure(r, fe->batch_pairs, fe->slot_mode, 0);
    rc = fq_fastq_resume(r, file_off, text.data(), text.size(), F.records_done, names.empty() ? nullptr : names.data(), bases.empty() ? nullptr : bases.data(), lens.empty() ? nullptr : lens.data(), F.shorter_after_longer);
    if (rc) { fq_fastq_close(r); return rc; }
    out[e] = r;
  }
  return FQ_OK;
}
extern "C" int fq_frontend_unequal_lengths(const fq_frontend_t *fe) { return fe && (fe->f[0].shorter_after_longer || fe->f[1].shorter_after_longer) ? 1 : 0; }
extern "C" void fq_frontend_stats(const fq_frontend_t *fe, fq_frontend_stats_t *s) {
  if (!fe || !s) return;
  s->ms_inflate = fe->ms_inflate; s->ms_tokenise = fe->ms_tokenise; s->members = fe->n_members; s->refused = fe->n_refused;
  s->text_bytes = fe->text_bytes; s->comp_bytes = fe->comp_bytes; s->pairs = fe->pairs_done;
  s->ms_wait_reader = fe->ms_wait_reader; s->ms_wait_slot = fe->ms_wait_slot; s->ms_read = fe->f[0].ms_read + fe->f[1].ms_read; s->ms_upload = fe->f[0].ms_upload + fe->f[1].ms_upload;
  s->ms_lines = fe->ms_lines; s->ms_records = fe->ms_records; s->ms_slots = fe->ms_slots; s->inflate_launches = fe->n_launch_inflate; s->chunks = fe->n_chunks;
  s->bam_records = fe->bam.records; s->bam_skipped = fe->bam.skipped; s->chain_repairs = fe->bam.repairs;
  s->bam_orphans = fe->bam.K.orphans; s->bam_held_peak_records = fe->bam.K.peak_n; s->bam_held_peak_bytes = fe->bam.K.peak_bytes;
  s->ms_bam_collate = fe->bam.K.ms[0] + fe->bam.K.ms[1] + fe->bam.K.ms[2] + fe->bam.K.ms[3] + fe->bam.K.ms[4];
  s->ms_bam_starts = fe->bam.ms_starts; s->ms_bam_pairs = fe->bam.ms_pairs; s->ms_bam_fill = fe->bam.ms_fill; s->ms_transcode = s->ms_bam_starts + s->ms_bam_pairs + s->ms_bam_fill;
  s->bam_unselected = fe->bam.unselected; s->bam_oq_records = fe->bam.oq_records; s->ms_bam_tags = fe->bam.ms_tags; s->bam_empty_chunks = fe->bam.empty_chunks;
}
// batch accessors
extern "C" int32_t fq_text_batch_pairs(const fq_text_batch_t *b) { return b ? b->n_pairs : 0; }
extern "C" const char *fq_text_batch_first_name(const fq_text_batch_t *b, int32_t sub_batch, int32_t end) {
  if (!b || sub_batch < 0 || end < 0 || end > 1 || (size_t)(((size_t)sub_batch * 2 + end + 1) * b->name_stride) > b->first_names.size()) return nullptr;
  return &b->first_names[((size_t)sub_batch * 2 + end) * b->name_stride];
}

// The batch's per-read arrays copied to the host (tests): head [3][rows] as fq_packed_batch_t::head, len [rows], names [rows][name_stride];
// rows = 2 * pairs (pairs for a single-end batch).  Returns the name stride, or a negative code.
extern "C" int fq_text_batch_fetch(fq_frontend_t *fe, const fq_text_batch_t *b, uint64_t *head, uint16_t *len, char *names, int64_t names_cap) {
  if (!fe || !b) return FQ_EINVAL;
  const size_t rows = (size_t)b->n_pairs * (b->single_end ? 1 : 2);
  DevScope scope(fe->device);                                  // (a state of this call's own: the readers' and the producer's are their threads')
  if (!scope.s || fqdev::bind(scope.s)) return FQ_ENODEV;
  if (head && fqdev::d2h(head, b->d_head, rows * 24)) return FQ_ENODEV;
  if (len && fqdev::d2h(len, b->d_hlen, rows * 2)) return FQ_ENODEV;
  if (names) { if ((int64_t)(rows * (size_t)b->name_stride) > names_cap) return FQ_ELIMIT; if (fqdev::d2h(names, b->d_names, rows * (size_t)b->name_stride)) return FQ_ENODEV; }
  if (fqdev::sync()) return FQ_ENODEV;
  return b->name_stride;
}
