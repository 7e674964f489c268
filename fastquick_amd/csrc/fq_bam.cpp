// fq_bam.cpp -- the BAM consumer of the alignment records: BwtMapper::SetSamRecord (src/BwtMapper.cpp:977-1264, the BAM_DEBUG
// branches that are compiled in: :946) and SetSamFileHeader (:947-975), written as BAM through an own BGZF layer (zlib raw deflate
// in 64 KB blocks).  Unlike the --sam_out dialect the records carry GENOME coordinates: a reduced-reference contig is named
// CHR:POS@REF/ALT[|L], the record's RNAME is CHR and its position POS - flank + offset-in-contig - 1 (:1026-1043), the header's
// @SQ lines are the original reference's (.fai), and every record carries RG:Z.  The record itself is fq_emit.h's fq_bam_record, the
// routine the consumers' kernels run: the host formatter loops over it on the host's view of the call (fq_ctx_host_view).
// fq_bam_create_sorted: the same records as a coordinate-sorted file with its .bai (what the pipeline's samtools sort / index steps make of O.bam, bin/FASTQuick_template.sh:501-502).
// The records are kept as runs until the close, which sorts all keys on the device (fq_sort.h) and emits in that order.  Runs that a call sorted on the device are read front
// to back by the emission; runs handed over as bytes (host formatter, fq_bam_write_records, the part files of --devices) are read at random -- fine in memory, slow from a
// spill file (a pread per record).
#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fastquick_amd.h"
#include "fq_index.h"
#include "fq_kernels.h"
#include "fq_pipeline.h"
#include "fq_backend.h"
#include <mutex>

// What the reference's translation unit sees as PACKAGE_VERSION when SetSamFileHeader is compiled: libbwa's 0.0.1 (bwase.h, included
// first), not src/Version.h's 1.0.6 -- the header the reference writes says VN:0.0.1 (oracle/_ref/fq_ref_driver --bam_dump).
#define FQ_PACKAGE_VERSION "0.0.1"

namespace {
// ---- BGZF (SAM/BAM specification 4.1): gzip members with a BC extra field, at most 64 KB of payload each ----------------------
struct Bgzf {
  // BGZF blocks are compressed independently (a fresh deflate stream each), so a run of them goes through zlib on several threads and
  // comes out byte for byte what one thread would write: the block boundaries (every 0xff00 bytes of the record stream) do not move.
  FILE *fp = nullptr;
  std::vector<uint8_t> buf;
  bool ok = true;
  static const size_t kBlock = 0xff00;
  static const int kThreads = 8;
  struct Out { uint8_t d[0x10000 + 64]; size_t n = 0; };
  static bool compress_block(const uint8_t *data, size_t n, Out &o) {
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    zs.next_in = const_cast<uint8_t *>(data); zs.avail_in = (uInt)n;
    zs.next_out = o.d + 18; zs.avail_out = sizeof o.d - 18 - 8;
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) { deflateEnd(&zs); return false; }
    const size_t clen = zs.total_out;
    deflateEnd(&zs);
    const size_t bsize = clen + 18 + 8;
    const uint8_t hdr[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, (uint8_t)((bsize - 1) & 0xff), (uint8_t)((bsize - 1) >> 8)};
    memcpy(o.d, hdr, 18);
    const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), data, (uInt)n), isz = (uint32_t)n;
    memcpy(o.d + 18 + clen, &crc, 4);
    memcpy(o.d + 18 + clen + 4, &isz, 4);
    o.n = bsize;
    return true;
  }
  void flush_blocks(size_t n_blocks, size_t last_len) {   // the first n_blocks - 1 blocks are full; the last holds last_len bytes
    if (!n_blocks) return;
    std::vector<Out> outs(n_blocks);
    std::vector<char> good(n_blocks, 0);
    auto work = [&](size_t lo, size_t hi) {
      for (size_t b = lo; b < hi; ++b) good[b] = compress_block(buf.data() + b * kBlock, b + 1 == n_blocks ? last_len : kBlock, outs[b]);
    };
    const size_t T = std::min<size_t>(kThreads, n_blocks);
    if (T <= 1) work(0, n_blocks);
    else {
      std::vector<std::thread> th;
      const size_t per = (n_blocks + T - 1) / T;
      for (size_t t = 0; t < T; ++t) { const size_t lo = t * per, hi = std::min(n_blocks, lo + per); if (lo < hi) th.emplace_back(work, lo, hi); }
      for (auto &x : th) x.join();
    }
    for (size_t b = 0; b < n_blocks; ++b) { if (!good[b] || fwrite(outs[b].d, 1, outs[b].n, fp) != outs[b].n) ok = false; }
  }
  void write(const void *p, size_t n) {
    const uint8_t *s = (const uint8_t *)p;
    buf.insert(buf.end(), s, s + n);
    if (buf.size() >= kBlock * 64) {                    // a few MB at a time
      const size_t nb = buf.size() / kBlock;
      flush_blocks(nb, kBlock);
      buf.erase(buf.begin(), buf.begin() + nb * kBlock);
    }
  }
  void flush_all() {                 // what is buffered goes out as blocks now (members made elsewhere follow)
    const size_t nb = (buf.size() + kBlock - 1) / kBlock;
    if (nb) flush_blocks(nb, buf.size() - (nb - 1) * kBlock);
    buf.clear();
  }
  void write_members(const void *p, size_t n) { if (n && fwrite(p, 1, n, fp) != n) ok = false; }
  void close() {
    if (!fp) return;
    const size_t nb = (buf.size() + kBlock - 1) / kBlock;
    if (nb) flush_blocks(nb, buf.size() - (nb - 1) * kBlock);
    buf.clear();
    Out eof;
    if (!compress_block(nullptr, 0, eof) || fwrite(eof.d, 1, eof.n, fp) != eof.n) ok = false;   // the empty end-of-file block
    fclose(fp);
    fp = nullptr;
  }
};

// ---- the sorted writer's runs (fq_bam_create_sorted) -------------------------------------------------------------------------
// One run per fq_bam_add_last / fq_bam_write_records: the record bytes and one FqBamSortEnt per record (fq_sort.h).  A run an attached context sorted on
// the device arrives in key order with its entries and is read front to back by the emission; a run handed over as bytes stays in input order, its
// entries come from the host loop over fq_bam_sort_entry, and the emission reads it at random -- fine in memory, slow from a spill file (a pread per record).
struct SortRun {
  std::vector<uint8_t> bytes;            // (empty when the run went to a file)
  std::vector<FqBamSortEnt> ent;
  std::vector<uint64_t> off;             // made at close: where each record begins in the run
  uint64_t n_bytes = 0;
  bool device_sorted = false;
  int fd = -1;
  std::string path;
};
struct SortWriter {
  std::string path;
  uint64_t mem_limit = 0, mem_used = 0, records = 0;
  int n_ref = 0, pos_bits = 1, key_bits = 2, n_tmp = 0;
  std::vector<SortRun> runs;
  fq_bam_sort_stats_t st{};
  fq_bam_sort_stats_t *at_close = nullptr;
  ~SortWriter() { for (SortRun &r : runs) { if (r.fd >= 0) ::close(r.fd); if (!r.path.empty()) ::unlink(r.path.c_str()); } }      // (also after a failed close)
};
static int bit_length(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }
static double now_sec() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

struct fq_bam {
  std::unique_ptr<SortWriter> sort;      // fq_bam_create_sorted: the records are kept as runs and leave at close
  // the formatter's tables (fq_emit.h: FqBamArgs): per contig the BAM reference id of its chromosome and where it lies in the genome;
  // made with the writer, uploaded when the first call formats on the device
  std::vector<int32_t> ctg_rid, ctg_g0;
  std::mutex dev_mu;
  bool dev_on = false;
  bool host_deflate = [] { const char *e = getenv("FASTQUICK_BAM_HOST_DEFLATE"); return e && *e && *e != '0'; }();   // A/B: zlib on the host's threads for device-formatted records too
  // how the device compresses (fq_deflate.h): FQ_DEFLATE_FIXED, or FQ_DEFLATE_DYNAMIC -- the block type chosen per member; fq_bam_set_deflate wins over the variable
  int deflate_mode = [] { const char *e = getenv("FASTQUICK_BAM_DEFLATE"); return e && !strcmp(e, "dynamic") ? FQ_DEFLATE_DYNAMIC : FQ_DEFLATE_FIXED; }();
  bool taken = false;                                    // records have been taken: the mode stays
  fq_bam_deflate_stats_t zst{};                          // the device's members by block type (counted in dynamic mode, from byte 18 of each as it is written)
  fq_bam_deflate_stats_t *zst_at_close = nullptr;
  uint8_t mem_hdr[19]; int mem_have = 0; uint64_t mem_skip = 0;
  void count_members(const uint8_t *p, size_t n) {       // a stretch of the members' bytes, cut anywhere
    while (n) {
      if (mem_skip) { const size_t k = (size_t)std::min<uint64_t>(mem_skip, n); p += k; n -= k; mem_skip -= k; continue; }
      mem_hdr[mem_have++] = *p++; --n;
      if (mem_have == 19) {
        ++((mem_hdr[18] >> 1 & 3) == 2 ? zst.members_dynamic : zst.members_fixed);
        mem_skip = (uint64_t)(mem_hdr[16] | mem_hdr[17] << 8) + 1 - 19; mem_have = 0;
      }
    }
  }
  std::vector<void *> d_bufs;
  const int32_t *d_rid = nullptr, *d_g0 = nullptr;
  const char *d_rg = nullptr;
  ~fq_bam() { for (void *p : d_bufs) fqdev::dfree(p); }
  const fq_index *ix = nullptr;
  fq_qc_opts_t o{};
  Bgzf z;
  std::vector<uint8_t> last;                             // the records of the last batch the host formatter made, or fq_bam_format_last fetched
  std::string err, rg_id, header_text;
  std::vector<std::pair<std::string, int>> contigs;      // BwtIndexer::contigSize
  std::map<std::string, int> ref_id;

  // genome coordinate of offset `pos1` (1-based) in reduced contig `seqid` (:1026-1043)
  void genome_coord(int seqid, int pos1, std::string *chrom, int *start) const {
    const std::string &name = ix->contigs[seqid].name;
    const size_t at = name.find('@'), colon = name.find(':');
    *chrom = name.substr(0, colon);
    const int refCoord = (int)strtol(name.substr(colon + 1, at - colon + 1).c_str(), nullptr, 10);
    *start = refCoord - (name.back() == 'L' ? o.flank_long_len : o.flank_len) + pos1 - 1;
  }
  int id_of(const std::string &chrom) const { auto it = ref_id.find(chrom); return it == ref_id.end() ? -1 : it->second; }
};

static int bam_create(const fq_index_t *ix, const char *fai_path, const char *bam_path, const char *rg_line, const fq_qc_opts_t *o, bool sorted, int64_t sort_mem, fq_bam_t **out) {
  if (!ix || !fai_path || !o || !out || (sorted && (!bam_path || sort_mem < 0))) return FQ_EINVAL;
  *out = nullptr;
  fq_bam *b = new fq_bam;
  b->ix = ix; b->o = *o;
  std::ifstream fai(fai_path);
  if (!fai.is_open()) { delete b; return FQ_EIO; }
  std::string line;
  while (std::getline(fai, line)) {   // BwtIndexer::LoadContigSize, src/BwtIndexer.cpp:771-781
    std::stringstream ss(line);
    std::string chr, length;
    ss >> chr;
    if (chr.empty()) continue;
    if (chr.find("chr") != std::string::npos || chr.find("CHR") != std::string::npos) chr = chr.substr(3);
    ss >> length;
    b->contigs.emplace_back(chr, atoi(length.c_str()));
  }
  // SetSamFileHeader (:947-975): @PG, the @RG line as given (tags in the order of the line), one @SQ per contig of the .fai
  std::ostringstream h;
  h << "@PG\tID:FASTQuick\tVN:" << FQ_PACKAGE_VERSION << "\n";
  const std::string rg = rg_line ? rg_line : "";
  if (rg.compare(0, 3, "@RG") == 0) {
    std::string esc;   // bwa_escape: "\t" written as two characters becomes a tab
    for (size_t i = 0; i < rg.size(); ++i) { if (rg[i] == '\\' && i + 1 < rg.size() && rg[i + 1] == 't') { esc += '\t'; ++i; } else esc += rg[i]; }
    const size_t idp = esc.find("\tID:");
    if (idp != std::string::npos) { size_t e = idp + 4; while (e < esc.size() && esc[e] != '\t' && esc[e] != '\n') ++e; b->rg_id = esc.substr(idp + 4, e - idp - 4); }
    std::stringstream toks(esc);
    std::string tok, id_field, rest;
    while (toks >> tok) {
      if (tok == "@RG") continue;
      if (tok.compare(0, 3, "ID:") == 0) id_field = tok; else rest += "\t" + tok;
    }
    if (!b->rg_id.empty()) h << "@RG\t" << (id_field.empty() ? "ID:" + b->rg_id : id_field) << rest << "\n";
  }
  for (size_t i = 0; i < b->contigs.size(); ++i) {
    h << "@SQ\tSN:" << b->contigs[i].first << "\tLN:" << b->contigs[i].second << "\n";
    b->ref_id.emplace(b->contigs[i].first, (int)i);   // (a repeated name keeps its first id)
  }
  b->header_text = h.str();
  for (size_t i = 0; i < ix->contigs.size(); ++i) {
    std::string chrom; int start;
    b->genome_coord((int)i, 1, &chrom, &start);        // start = refCoord - flank + 1 - 1
    b->ctg_rid.push_back(b->id_of(chrom)); b->ctg_g0.push_back(start);
  }
  b->ctg_rid.push_back(-1); b->ctg_g0.push_back(0);      // (one entry behind the last contig, as the tables always had)
  if (!bam_path) { *out = b; return FQ_OK; }          // a formatter without a file (fq_bam_format_last)
  b->z.fp = fopen(bam_path, "wb");
  if (!b->z.fp) { delete b; return FQ_EIO; }
  if (sorted) {
    b->header_text = "@HD\tVN:1.6\tSO:coordinate\n" + b->header_text;
    b->sort.reset(new SortWriter);
    SortWriter &S = *b->sort;
    S.path = bam_path; S.mem_limit = (uint64_t)sort_mem; S.n_ref = (int)b->contigs.size();
    int max_ln = 0;
    for (const auto &cg : b->contigs) max_ln = std::max(max_ln, cg.second);
    S.pos_bits = std::max(1, bit_length((uint64_t)max_ln + 1));      // room for max LN + 1 and for n_ref: the key's width needs no reduction on the device
    S.key_bits = std::max(1, bit_length((uint64_t)S.n_ref)) + S.pos_bits + 1;
    S.st.key_bits = S.key_bits; S.st.pos_bits = S.pos_bits;
  }
  const int32_t l_text = (int32_t)b->header_text.size(), n_ref = (int32_t)b->contigs.size();
  b->z.write("BAM\1", 4);
  b->z.write(&l_text, 4);
  b->z.write(b->header_text.data(), b->header_text.size());
  b->z.write(&n_ref, 4);
  for (const auto &cg : b->contigs) {
    const int32_t l_name = (int32_t)cg.first.size() + 1, l_ref = cg.second;
    b->z.write(&l_name, 4);
    b->z.write(cg.first.c_str(), (size_t)l_name);
    b->z.write(&l_ref, 4);
  }
  *out = b;
  return FQ_OK;
}
extern "C" int fq_bam_create(const fq_index_t *ix, const char *fai_path, const char *bam_path, const char *rg_line, const fq_qc_opts_t *o, fq_bam_t **out) {
  return bam_create(ix, fai_path, bam_path, rg_line, o, false, 0, out);
}
extern "C" int fq_bam_create_sorted(const fq_index_t *ix, const char *fai_path, const char *bam_path, const char *rg_line, const fq_qc_opts_t *o, int64_t sort_mem_bytes, fq_bam_t **out) {
  return bam_create(ix, fai_path, bam_path, rg_line, o, true, sort_mem_bytes, out);
}

bool fq_bam_sort_params(const fq_bam *b, int *n_ref, int *pos_bits, int *key_bits) {
  if (!b || !b->sort) return false;
  *n_ref = b->sort->n_ref; *pos_bits = b->sort->pos_bits; *key_bits = b->sort->key_bits;
  return true;
}
bool fq_bam_wants_members(const fq_bam *b) { return b->z.fp != nullptr && !b->host_deflate && !b->sort; }      // (a sorted writer compresses once, behind the merge)
int fq_bam_deflate_mode(const fq_bam *b) { return b->deflate_mode; }
extern "C" int fq_bam_set_deflate(fq_bam_t *b, int mode) {
  if (!b || (mode != FQ_DEFLATE_FIXED && mode != FQ_DEFLATE_DYNAMIC) || b->taken) return FQ_EINVAL;
  b->deflate_mode = mode;
  return FQ_OK;
}
extern "C" int fq_bam_deflate_stats(const fq_bam_t *b, fq_bam_deflate_stats_t *out) {
  if (!b || !out) return FQ_EINVAL;
  *out = b->zst; out->mode = b->deflate_mode;
  return FQ_OK;
}
extern "C" int fq_bam_deflate_stats_at_close(fq_bam_t *b, fq_bam_deflate_stats_t *out) {
  if (!b) return FQ_EINVAL;
  b->zst_at_close = out;
  return FQ_OK;
}
// the formatter's part of a call's kernel arguments (on the calling context's bound state)
int fq_bam_device_prepare(fq_bam *b, FqBamArgs *a) {
  std::lock_guard<std::mutex> lk(b->dev_mu);
  if (!b->dev_on) {
    bool ok = true;
    auto up = [&](const void *src, size_t bytes) -> void * {
      void *d = fqdev::dmalloc(bytes ? bytes : 16);
      if (!d) { ok = false; return nullptr; }
      b->d_bufs.push_back(d);
      if (bytes && fqdev::h2d(d, src, bytes)) ok = false;
      return d;
    };
    b->d_rid = (const int32_t *)up(b->ctg_rid.data(), b->ctg_rid.size() * 4); b->d_g0 = (const int32_t *)up(b->ctg_g0.data(), b->ctg_g0.size() * 4);
    b->d_rg = (const char *)up(b->rg_id.c_str(), b->rg_id.size() + 1);
    if (!ok || fqdev::sync()) return FQ_ENODEV;
    b->dev_on = true;
  }
  a->ctg_rid = b->d_rid; a->ctg_g0 = b->d_g0; a->rg = b->d_rg; a->rg_len = (int32_t)b->rg_id.size();
  return FQ_OK;
}

// the BAM branch of PairEndMapper's consumer loop over one batch (src/BwtMapper.cpp:2054-2085): the batch's records, in input order, in b->last
static int format_last(fq_bam_t *b, fq_ctx_t *c) {
  FqBamArgs A{};
  if (const int rc = fq_ctx_host_view(c, &A.s)) { b->err = fq_ctx_last_error(c); return rc; }
  A.ctg_rid = b->ctg_rid.data(); A.ctg_g0 = b->ctg_g0.data(); A.rg = b->rg_id.c_str(); A.rg_len = (int32_t)b->rg_id.size();
  const size_t N = 2 * (size_t)A.s.n_surv;
  std::vector<uint32_t> len(N + 1), meta(N + 1);
  std::vector<uint64_t> off(N + 1);
  A.len = len.data(); A.meta = meta.data(); A.off = off.data(); A.split = 0;
  fq_host_records(A.s.n_surv, [&](int idx) { fq_bam_len_thread(A, idx); });
  uint64_t total = 0;
  for (size_t i = 0; i < N; ++i) { off[i] = total; total += len[i]; }
  b->last.resize((size_t)total);
  A.out = b->last.data();
  fq_host_records(A.s.n_surv, [&](int idx) { fq_bam_fill_thread(A, idx); });
  return FQ_OK;
}
// ---- sorted writer: taking runs --------------------------------------------------------------------------------------------------
// `len` bytes of whole records as one run; ents: the entries that came with them from the device (then the records are in key order), or nullptr
// take: the vector that holds data, which the run keeps instead of copying it (or nullptr)
static int sort_add_run(fq_bam_t *b, const uint8_t *data, uint64_t len, const FqBamSortEnt *ents, uint64_t n_ents, std::vector<uint8_t> *take = nullptr) {
  SortWriter &S = *b->sort;
  SortRun run;
  run.n_bytes = len;
  if (ents) {
    for (uint64_t i = 0; i < n_ents; ++i) if (ents[i].len) run.ent.push_back(ents[i]);      // (a single-end call keeps the pair layout: its second records are empty)
    run.device_sorted = true;
    uint64_t sum = 0;
    for (const FqBamSortEnt &e : run.ent) sum += e.len;
    if (sum != len) { b->err = "sorted BAM: a device-sorted run's entries do not add up to its bytes"; return FQ_EINVAL; }
  }
  else {
    for (uint64_t p = 0; p < len;) {      // the host loop over the body launch_bam_key runs
      if (len - p < 4) { b->err = "sorted BAM: a run does not end with a whole record"; return FQ_EINVAL; }
      const uint64_t rl = (uint64_t)fq_sort_ld32(data + p) + 4;
      if (rl < 36 || rl > len - p) { b->err = "sorted BAM: a run does not hold whole records"; return FQ_EINVAL; }
      run.ent.push_back(fq_bam_sort_entry(data + p, (uint32_t)rl, S.n_ref, S.pos_bits));
      p += rl;
    }
  }
  if (S.records + run.ent.size() > 0xffffffffull) { b->err = "sorted BAM: more than 2^32 - 1 records (the merge's ordinals are 32 bits wide)"; return FQ_ELIMIT; }
  if (len && S.mem_used + len > S.mem_limit) {      // raw into a file of its own, read back with pread at close
    char suffix[32];
    snprintf(suffix, sizeof suffix, ".tmp.%04d", S.n_tmp++);
    run.path = S.path + suffix;
    run.fd = ::open(run.path.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644);
    bool ok = run.fd >= 0;
    for (uint64_t p = 0; ok && p < len;) { const ssize_t w = ::write(run.fd, data + p, (size_t)std::min<uint64_t>(len - p, (uint64_t)1 << 30)); if (w <= 0) ok = false; else p += (uint64_t)w; }
    if (!ok) { if (run.fd >= 0) ::close(run.fd); ::unlink(run.path.c_str()); b->err = "sorted BAM: cannot write " + run.path; return FQ_EIO; }
    ::close(run.fd); run.fd = -1;      // (opened again for the close: a long job makes more runs than a process may hold files open)
    ++S.st.spilled_runs;
  } else if (len) { if (take) run.bytes = std::move(*take); else run.bytes.assign(data, data + len); S.mem_used += len; }
  S.records += run.ent.size();
  ++S.st.runs; S.st.device_sorted_runs += run.device_sorted ? 1 : 0; S.st.records = (int64_t)S.records;
  S.runs.push_back(std::move(run));
  return FQ_OK;
}
extern "C" int fq_bam_sort_stats(const fq_bam_t *b, fq_bam_sort_stats_t *out) {
  if (!b || !out || !b->sort) return FQ_EINVAL;
  *out = b->sort->st;
  return FQ_OK;
}
static_assert(sizeof(fq_bam_sort_ent_t) == sizeof(FqBamSortEnt), "the public entry is fq_sort.h's");
extern "C" int64_t fq_bam_sort_run_entries(const fq_bam_t *b, int64_t run, fq_bam_sort_ent_t *out, int64_t cap) {
  if (!b || !b->sort || cap < 0 || (cap > 0 && !out)) return FQ_EINVAL;
  const int64_t n_runs = (int64_t)b->sort->runs.size();
  if (run < 0) run += n_runs;
  if (run < 0 || run >= n_runs) return FQ_EINVAL;
  const std::vector<FqBamSortEnt> &e = b->sort->runs[(size_t)run].ent;
  if (!e.empty() && cap > 0) memcpy(out, e.data(), (size_t)std::min<int64_t>(cap, (int64_t)e.size()) * sizeof(FqBamSortEnt));
  return (int64_t)e.size();
}
extern "C" int fq_bam_sort_stats_at_close(fq_bam_t *b, fq_bam_sort_stats_t *out) {
  if (!b || !b->sort) return FQ_EINVAL;
  b->sort->at_close = out;
  return FQ_OK;
}

// ---- the device's part of the sort and of the close: one bound state, its buffers kept for as long as the scope lives ------------------------------
namespace {
struct DevScope {
  fqdev::State *s = nullptr;
  std::vector<void *> d, h;
  explicit DevScope(int device) : s(fqdev::state_create(device)) {}
  bool bind() { return s && !fqdev::bind(s); }
  template <class T> T *dm(size_t n) { void *p = fqdev::dmalloc(n * sizeof(T)); if (p) d.push_back(p); return (T *)p; }
  template <class T> T *hm(size_t n) { void *p = fqdev::hmalloc(n * sizeof(T)); if (p) h.push_back(p); return (T *)p; }
  void release(void *p) { auto it = std::find(d.begin(), d.end(), p); if (it != d.end()) { fqdev::dfree(p); d.erase(it); } }
  ~DevScope() { if (s) { (void)fqdev::bind(s); (void)fqdev::sync(); } for (void *p : d) fqdev::dfree(p); for (void *p : h) fqdev::hfree(p); fqdev::state_destroy(s); }
};
// perm[i] = the place in keys of the i-th key in stable ascending order (on the bound state; its buffers are freed again)
int sort_keys_bound(DevScope &D, const uint64_t *keys, uint32_t n, int key_bits, uint32_t *perm, double *kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  if (!n) return FQ_OK;
  const size_t nh = (size_t)FQ_SORT_DIGITS * fq_sort_tiles(n);
  uint64_t *k_in = D.dm<uint64_t>(n), *k_out = D.dm<uint64_t>(n), *k_tmp = D.dm<uint64_t>(n), *hoff = D.dm<uint64_t>(nh + 2);
  uint32_t *p_out = D.dm<uint32_t>(n), *p_tmp = D.dm<uint32_t>(n), *hist = D.dm<uint32_t>(nh + 1);
  int rc = FQ_OK;
  if (!k_in || !k_out || !k_tmp || !hoff || !p_out || !p_tmp || !hist) rc = FQ_ENOMEM;
  else {
    const FqSortScratch sc{k_tmp, p_tmp, hist, hoff};
    if (fqdev::h2d(k_in, keys, (size_t)n * 8) || fqdev::launch_sort_pairs(k_in, n, key_bits, k_out, p_out, sc) || fqdev::d2h(perm, p_out, (size_t)n * 4) || fqdev::sync()) rc = FQ_ENODEV;
    double ms[FQ_KX_COUNT] = {0}; uint64_t ln[FQ_KX_COUNT] = {0};
    fqdev::time_collect(ms, ln, FQ_KX_COUNT);
    if (kernel_ms) *kernel_ms = ms[FQ_KX_SORT];
  }
  for (void *p : {(void *)k_in, (void *)k_out, (void *)k_tmp, (void *)hoff, (void *)p_out, (void *)p_tmp, (void *)hist}) D.release(p);
  return rc;
}
// reg2bin of the SAM specification (5.3): the bin of the zero-based half-open interval [beg, end)
int reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}
void put32(std::vector<uint8_t> &v, uint32_t x) { for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> (8 * k))); }
void put64(std::vector<uint8_t> &v, uint64_t x) { for (int k = 0; k < 8; ++k) v.push_back((uint8_t)(x >> (8 * k))); }
}  // namespace

extern "C" int fq_sort_keys_device(int device, const uint64_t *keys, int64_t n, int key_bits, uint32_t *perm, double *kernel_ms) {
  if (n < 0 || n > 0xffffffffll || key_bits < 1 || key_bits > 64 || (n > 0 && (!keys || !perm))) return FQ_EINVAL;
  DevScope D(device);
  if (!D.bind()) return FQ_ENODEV;
  return sort_keys_bound(D, keys, (uint32_t)n, key_bits, perm, kernel_ms);
}

// ---- sorted writer: the close ------------------------------------------------------------------------------------------------------
// The total order is the device's sort again: the runs' keys behind each other in run order, sorted stably with the global ordinal as payload, so that
// ties fall in input order across runs (no heap merge on the host).  The header's members have gone through the host BGZF layer; the merged record stream
// is assembled in slices of whole members by several threads (each a contiguous range of output bytes), compressed by the compressor the unsorted writer
// uses -- the device's members, or zlib under FASTQUICK_BAM_HOST_DEFLATE -- on ONE device state that lives for the whole close, and written in order.
// The index's virtual offsets come from the BSIZE fields of the members that came back.
static int sort_close(fq_bam_t *b) {
  SortWriter &S = *b->sort;
  const double t_begin = now_sec();
  const uint64_t N = S.records;
  DevScope D(b->ix->device);
  if (!D.bind()) { b->err = std::string("sorted BAM: ") + fqdev::last_error(); return FQ_ENODEV; }
  for (SortRun &R : S.runs)
    if (!R.path.empty() && (R.fd = ::open(R.path.c_str(), O_RDONLY)) < 0) { b->err = "sorted BAM: cannot open " + R.path + " again"; return FQ_EIO; }
  // 1. the order
  std::vector<uint64_t> run_base(S.runs.size() + 1, 0);
  std::vector<uint32_t> perm((size_t)N);
  {
    std::vector<uint64_t> keys((size_t)N);
    uint64_t g = 0;
    for (size_t r = 0; r < S.runs.size(); ++r) {
      SortRun &R = S.runs[r];
      run_base[r] = g;
      R.off.resize(R.ent.size() + 1);
      uint64_t o = 0;
      for (size_t j = 0; j < R.ent.size(); ++j) { keys[g++] = R.ent[j].key; R.off[j] = o; o += R.ent[j].len; }
      R.off[R.ent.size()] = o;
      if (o != R.n_bytes) { b->err = "sorted BAM: a run's entries do not add up to its bytes"; return FQ_EINVAL; }
    }
    run_base[S.runs.size()] = g;
    double ms = 0;
    const int rc = sort_keys_bound(D, keys.data(), (uint32_t)N, S.key_bits, perm.data(), &ms);
    if (rc) { b->err = std::string("sorted BAM: the key sort failed: ") + fqdev::last_error(); return rc; }
    S.st.sort_kernel_ms += ms;
  }
  const double t_sorted = now_sec();
  // 2. where every record of the output comes from and goes to
  std::vector<FqBamSortEnt> se((size_t)N);
  std::vector<uint32_t> src_run((size_t)N);
  std::vector<uint64_t> src_off((size_t)N), ooff((size_t)N + 1);
  std::vector<uint8_t> unmapped((size_t)N, 0);
  {
    uint64_t o = 0;
    for (uint64_t i = 0; i < N; ++i) {
      const uint64_t g = perm[i];
      const size_t r = (size_t)(std::upper_bound(run_base.begin(), run_base.end() - 1, g) - run_base.begin()) - 1;
      const SortRun &R = S.runs[r];
      se[i] = R.ent[g - run_base[r]]; src_run[i] = (uint32_t)r; src_off[i] = R.off[g - run_base[r]];
      ooff[i] = o; o += se[i].len;
    }
    ooff[N] = o;
  }
  std::vector<uint32_t>().swap(perm);
  const uint64_t total = ooff[N];
  // 3. the record stream, slice by slice
  b->z.flush_all();
  if (!b->z.ok) return FQ_EIO;
  uint64_t fpos = (uint64_t)ftello(b->z.fp);
  const uint64_t n_mem = (total + FQD_BLOCK - 1) / FQD_BLOCK;
  std::vector<uint64_t> member_off((size_t)n_mem + 1);
  const uint32_t SLB = 256;                                   // members per slice
  const size_t SL = (size_t)SLB * FQD_BLOCK;
  const bool on_device = !b->host_deflate, dynamic = b->deflate_mode == FQ_DEFLATE_DYNAMIC;
  uint8_t *p_in = D.hm<uint8_t>(SL + 64), *p_out = D.hm<uint8_t>((size_t)SLB * FQD_SLOT);
  uint8_t *d_in = nullptr, *d_stage = nullptr, *d_out = nullptr; uint32_t *d_bs = nullptr; uint64_t *d_off = nullptr;
  if (!p_in || !p_out) { b->err = "sorted BAM: out of pinned host memory"; return FQ_ENOMEM; }
  if (on_device && total) {
    d_in = D.dm<uint8_t>(SL + 64); d_stage = D.dm<uint8_t>((size_t)SLB * FQD_SLOT); d_out = D.dm<uint8_t>((size_t)SLB * FQD_SLOT);
    d_bs = D.dm<uint32_t>(SLB + 1); d_off = D.dm<uint64_t>(SLB + 2);
    if (!d_in || !d_stage || !d_out || !d_bs || !d_off) { b->err = "sorted BAM: out of device memory"; return FQ_ENOMEM; }
    if (!fqdev::crc_const()) { b->err = std::string("BGZF on the device: ") + fqdev::last_error(); return FQ_ENODEV; }
  }
  double t_assemble = 0, t_compress = 0;
  std::atomic<bool> read_bad{false};
  auto read_src = [&](uint64_t i, uint64_t at, uint64_t n, uint8_t *dst) {      // n bytes of output record i from byte `at` of it
    const SortRun &R = S.runs[src_run[i]];
    if (R.fd < 0) { memcpy(dst, R.bytes.data() + src_off[i] + at, (size_t)n); return; }
    for (uint64_t got = 0; got < n;) { const ssize_t k = ::pread(R.fd, dst + got, (size_t)(n - got), (off_t)(src_off[i] + at + got)); if (k <= 0) { read_bad = true; return; } got += (uint64_t)k; }
  };
  auto assemble = [&](uint64_t lo, uint64_t hi, uint64_t s0) {                   // output bytes [lo, hi) into p_in - s0
    uint64_t i = (uint64_t)(std::upper_bound(ooff.begin(), ooff.end(), lo) - ooff.begin()) - 1;
    for (uint64_t pos = lo; pos < hi; ++i) {
      const uint64_t at = pos - ooff[i], n = std::min(ooff[i + 1], hi) - pos;
      read_src(i, at, n, p_in + (pos - s0));
      if (at == 0) {                                                            // whoever copies a record's first byte notes its flag 4 for the index
        uint8_t f[2];
        if (n >= 20) memcpy(f, p_in + (pos - s0) + 18, 2); else read_src(i, 18, 2, f);
        unmapped[i] = (f[0] & 4) ? 1 : 0;
      }
      pos += n;
    }
  };
  for (uint64_t s0 = 0, m0 = 0; s0 < total; s0 += SL, m0 += SLB) {
    const uint64_t n = std::min<uint64_t>(SL, total - s0);
    const uint32_t nb = (uint32_t)((n + FQD_BLOCK - 1) / FQD_BLOCK);
    const double ta = now_sec();
    {
      const uint64_t T = std::min<uint64_t>(Bgzf::kThreads, (n + 65535) / 65536), per = (n + T - 1) / T;
      std::vector<std::thread> th;
      for (uint64_t t = 1; t < T; ++t) { const uint64_t lo = s0 + t * per, hi = std::min(s0 + n, lo + per); if (lo < hi) th.emplace_back(assemble, lo, hi, s0); }
      assemble(s0, std::min(s0 + n, s0 + per), s0);
      for (auto &x : th) x.join();
    }
    if (read_bad) { b->err = "sorted BAM: reading a spilled run back failed"; return FQ_EIO; }
    const double tc = now_sec();
    t_assemble += tc - ta;
    uint64_t zn = 0;
    if (on_device) {
      FqDeflateArgs a{d_in, n, d_stage, d_bs, fqdev::crc_const(), nb, d_out};      // (dynamic mode keeps its tokens where the pack writes afterwards)
      FqDeflatePackArgs pk{d_stage, d_bs, d_off, d_out, nb};
      if (fqdev::h2d(d_in, p_in, (size_t)n) || (dynamic ? fqdev::launch_deflate_dyn(a) : fqdev::launch_deflate(a)) || fqdev::launch_scan(d_bs, d_off, nb) || fqdev::launch_deflate_pack(pk) || fqdev::d2h(&zn, d_off + nb, 8) || fqdev::sync() ||
          zn > (uint64_t)SLB * FQD_SLOT || fqdev::d2h(p_out, d_out, (size_t)zn) || fqdev::sync()) { b->err = std::string("sorted BAM: BGZF on the device: ") + fqdev::last_error(); return FQ_ENODEV; }
    } else {
      std::vector<Bgzf::Out> outs(nb);
      std::vector<char> good(nb, 0);
      auto work = [&](uint32_t lo, uint32_t hi) { for (uint32_t k = lo; k < hi; ++k) good[k] = Bgzf::compress_block(p_in + (size_t)k * FQD_BLOCK, (size_t)std::min<uint64_t>(FQD_BLOCK, n - (uint64_t)k * FQD_BLOCK), outs[k]); };
      const uint32_t T = std::min<uint32_t>(Bgzf::kThreads, nb), per = (nb + T - 1) / T;
      std::vector<std::thread> th;
      for (uint32_t t = 0; t < T; ++t) { const uint32_t lo = t * per, hi = std::min(nb, lo + per); if (lo < hi) th.emplace_back(work, lo, hi); }
      for (auto &x : th) x.join();
      for (uint32_t k = 0; k < nb; ++k) { if (!good[k]) { b->err = "sorted BAM: zlib failed"; return FQ_EIO; } memcpy(p_out + zn, outs[k].d, outs[k].n); zn += outs[k].n; }
    }
    uint64_t p = 0;
    for (uint32_t k = 0; k < nb; ++k) {                        // the members' sizes as the file holds them: BSIZE
      if (p + 18 > zn) { b->err = "sorted BAM: the compressor returned fewer members than blocks"; return FQ_EIO; }
      member_off[(size_t)(m0 + k)] = fpos + p;
      p += (uint64_t)fq_sort_ld16(p_out + p + 16) + 1;
    }
    if (p != zn) { b->err = "sorted BAM: the members' sizes do not add up"; return FQ_EIO; }
    if (on_device && dynamic) b->count_members(p_out, (size_t)zn);
    b->z.write_members(p_out, (size_t)zn);
    if (!b->z.ok) return FQ_EIO;
    fpos += zn;
    t_compress += now_sec() - tc;
  }
  member_off[(size_t)n_mem] = fpos;
  const uint64_t eof_voff = fpos << 16;
  b->z.close();                                                // (nothing buffered: the end-of-file block)
  if (!b->z.ok) return FQ_EIO;
  const double t_written = now_sec();
  // 4. the index (SAM specification 5.2)
  auto voff = [&](uint64_t i) { return i >= N ? eof_voff : member_off[(size_t)(ooff[i] / FQD_BLOCK)] << 16 | ooff[i] % FQD_BLOCK; };
  std::vector<uint8_t> bai;
  bai.insert(bai.end(), {'B', 'A', 'I', 1});
  put32(bai, (uint32_t)S.n_ref);
  uint64_t i = 0, n_no_coor = 0;
  const uint64_t pos_mask = ((uint64_t)1 << S.pos_bits) - 1;
  for (int ref = 0; ref < S.n_ref; ++ref) {
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
    std::vector<uint64_t> lin;
    uint64_t off_beg = 0, off_end = 0, n_map = 0, n_unmap = 0;
    uint32_t last_bin = 0xffffffffu;
    bool any = false;
    for (; i < N && (int64_t)(se[i].key >> (S.pos_bits + 1)) == ref; ++i) {
      const int64_t beg = std::max<int64_t>((int64_t)(se[i].key >> 1 & pos_mask) - 1, 0), end = std::max<int64_t>(se[i].end, beg + 1);
      const uint64_t v0 = voff(i), v1 = voff(i + 1);
      const uint32_t bin = (uint32_t)reg2bin(beg, end);
      if (bin == last_bin) bins[bin].back().second = v1;        // consecutive records of one bin share a chunk
      else bins[bin].emplace_back(v0, v1);
      last_bin = bin;
      const size_t w1 = (size_t)((end - 1) >> 14);
      if (lin.size() <= w1) lin.resize(w1 + 1, 0);
      for (size_t w = (size_t)(beg >> 14); w <= w1; ++w) if (!lin[w]) lin[w] = v0;      // (offsets ascend: the first record seen is the smallest)
      if (!any) { off_beg = v0; any = true; }
      off_end = v1;
      if (unmapped[i]) ++n_unmap; else ++n_map;
    }
    for (size_t w = lin.size(); w-- > 1;) if (!lin[w - 1]) lin[w - 1] = lin[w];           // a window no record overlaps: the next later window's value
    put32(bai, (uint32_t)(bins.size() + (any ? 1 : 0)));
    for (const auto &kv : bins) {
      put32(bai, kv.first); put32(bai, (uint32_t)kv.second.size());
      for (const auto &c : kv.second) { put64(bai, c.first); put64(bai, c.second); }
    }
    if (any) { put32(bai, 37450); put32(bai, 2); put64(bai, off_beg); put64(bai, off_end); put64(bai, n_map); put64(bai, n_unmap); }
    put32(bai, (uint32_t)lin.size());
    for (uint64_t v : lin) put64(bai, v);
  }
  n_no_coor = N - i;
  put64(bai, n_no_coor);
  {
    const std::string path = S.path + ".bai";
    FILE *f = fopen(path.c_str(), "wb");
    const bool ok = f && fwrite(bai.data(), 1, bai.size(), f) == bai.size();
    if (f && fclose(f)) { b->err = "sorted BAM: cannot write " + path; return FQ_EIO; }
    if (!ok) { b->err = "sorted BAM: cannot write " + path; return FQ_EIO; }
  }
  const double t_end = now_sec();
  S.st.close_sec = t_end - t_begin; S.st.close_sort_sec = t_sorted - t_begin; S.st.close_assemble_sec = t_assemble; S.st.close_compress_sec = t_compress;
  S.st.close_index_sec = t_end - t_written;
  if (S.at_close) *S.at_close = S.st;
  return FQ_OK;
}

extern "C" int fq_bam_add_last(fq_bam_t *b, fq_ctx_t *c) {
  if (!b || !c || !b->z.fp) return FQ_EINVAL;
  b->taken = true;
  if (const FqBamCallOut *D = fq_ctx_bam_out(c)) {        // the records were formatted by the call's kernels (fq_ctx_attach_bam): they only leave the device here
    if (D->owner != b || !D->ready) { b->err = "fq_bam_add_last: the context's last call formatted its records for another writer, or failed"; return FQ_EINVAL; }
    if (fq_ctx_emit_wait(c)) { b->err = "fq_bam_add_last: waiting for the call's kernels failed"; return FQ_ENODEV; }      // (z_bytes comes back with them)
    if (b->sort) {          // a run of the sorted writer: the call sorted its records (emit_fill); they arrive in key order with their entries
      if (!D->sorted && D->bytes) { b->err = "fq_bam_add_last: the call left no sorted run"; return FQ_EINVAL; }
      const fq_sink_fn append = [](void *user, const void *d, int64_t l) -> int { auto *v = (std::vector<uint8_t> *)user; v->insert(v->end(), (const uint8_t *)d, (const uint8_t *)d + l); return 0; };
      std::vector<uint8_t> ent, rec;      // (rec becomes the run's bytes: fetched once, not copied again)
      if (D->bytes) {
        rec.reserve((size_t)D->bytes); ent.reserve((size_t)D->n_rec * sizeof(FqBamSortEnt));
        if (fq_ctx_bam_stream(c, append, &rec, FQ_BAM_STREAM_SORTED) < 0 || fq_ctx_bam_stream(c, append, &ent, FQ_BAM_STREAM_ENTRIES) < 0) { b->err = "fq_bam_add_last: fetching the sorted run from the device failed"; return FQ_ENODEV; }
      }
      b->sort->st.sort_kernel_ms += D->sort_ms; b->sort->st.gather_kernel_ms += D->gather_ms;
      static const FqBamSortEnt none{};      // (an empty call: a device-sorted run without records)
      return sort_add_run(b, rec.data(), rec.size(), ent.empty() ? &none : (const FqBamSortEnt *)ent.data(), ent.size() / sizeof(FqBamSortEnt), &rec);
    }
    int64_t n;
    if (D->z_bytes) {       // finished BGZF members (fq_deflate.h): appended behind whatever the host's layer still holds
      b->z.flush_all();
      n = fq_ctx_bam_stream(c, [](void *user, const void *data, int64_t len) -> int {
        fq_bam *w = (fq_bam *)user;
        if (w->deflate_mode == FQ_DEFLATE_DYNAMIC) w->count_members((const uint8_t *)data, (size_t)len);
        w->z.write_members(data, (size_t)len);
        return w->z.ok ? 0 : 1;
      }, b, FQ_BAM_STREAM_MEMBERS);
    } else n = fq_ctx_bam_stream(c, [](void *user, const void *data, int64_t len) -> int { ((fq_bam *)user)->z.write(data, (size_t)len); return ((fq_bam *)user)->z.ok ? 0 : 1; }, b, 0);
    if (n < 0) { b->err = "fq_bam_add_last: fetching the records from the device failed"; return (int)n; }
    return b->z.ok ? FQ_OK : FQ_EIO;
  }
  const int rc = format_last(b, c);
  if (rc) return rc;
  if (b->sort) return sort_add_run(b, b->last.data(), b->last.size(), nullptr, 0);
  if (!b->last.empty()) b->z.write(b->last.data(), b->last.size());
  return b->z.ok ? FQ_OK : FQ_EIO;
}
// The same records as bytes (uncompressed BAM records, block_size first), for a caller that writes them itself or elsewhere: several
// devices format the batches of their FASTQ pairs at once and one writer appends them in input order (fq_bam_write_records).
extern "C" int fq_bam_format_last(fq_bam_t *b, fq_ctx_t *c, const void **data, int64_t *len) {
  if (!b || !c || !data || !len) return FQ_EINVAL;
  if (const FqBamCallOut *D = fq_ctx_bam_out(c)) {
    if (D->owner != b || !D->ready) { b->err = "fq_bam_format_last: the context's last call formatted its records for another writer, or failed"; return FQ_EINVAL; }
    b->last.clear();
    b->last.reserve((size_t)D->bytes);
    const int64_t n = fq_ctx_bam_stream(c, [](void *user, const void *d, int64_t l) -> int { auto *v = (std::vector<uint8_t> *)user; v->insert(v->end(), (const uint8_t *)d, (const uint8_t *)d + l); return 0; }, &b->last, 0);
    if (n < 0) return (int)n;
    *data = b->last.data(); *len = (int64_t)b->last.size();
    return FQ_OK;
  }
  const int rc = format_last(b, c);
  if (rc) return rc;
  *data = b->last.data(); *len = (int64_t)b->last.size();
  return FQ_OK;
}
extern "C" int fq_bam_write_records(fq_bam_t *b, const void *data, int64_t len) {
  if (!b || !b->z.fp || len < 0 || (len > 0 && !data)) return FQ_EINVAL;
  b->taken = true;
  if (b->sort) return sort_add_run(b, (const uint8_t *)data, (uint64_t)len, nullptr, 0);
  if (len) b->z.write(data, (size_t)len);
  return b->z.ok ? FQ_OK : FQ_EIO;
}
// (tests, tools) n bytes as BGZF members written by the device's compressor (fq_deflate.h): the members behind each other into out (capacity cap);
// *out_len their size, *kernel_ms the compressor kernel's time.  FQ_ELIMIT when cap is too small.
// mode: FQ_DEFLATE_*
extern "C" int fq_bgzf_deflate_device_mode(int device, int mode, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *out_len, double *kernel_ms) {
  if (!in || !out || !out_len || n < 0 || (mode != FQ_DEFLATE_FIXED && mode != FQ_DEFLATE_DYNAMIC)) return FQ_EINVAL;
  struct DevScope { fqdev::State *s; ~DevScope() { fqdev::state_destroy(s); } } scope{fqdev::state_create(device)};
  if (!scope.s || fqdev::bind(scope.s)) return FQ_ENODEV;
  const uint32_t nb = (uint32_t)((n + FQD_BLOCK - 1) / FQD_BLOCK);
  *out_len = 0;
  if (kernel_ms) *kernel_ms = 0;
  if (!nb) return FQ_OK;
  uint8_t *d_in = (uint8_t *)fqdev::dmalloc((size_t)n + 64), *d_stage = (uint8_t *)fqdev::dmalloc((size_t)nb * FQD_SLOT), *d_out = (uint8_t *)fqdev::dmalloc((size_t)nb * FQD_SLOT);
  uint32_t *d_bs = (uint32_t *)fqdev::dmalloc(((size_t)nb + 1) * 4);
  uint64_t *d_off = (uint64_t *)fqdev::dmalloc(((size_t)nb + 2) * 8);
  int rc = FQ_OK;
  uint64_t total = 0;
  if (!d_in || !d_stage || !d_out || !d_bs || !d_off) rc = FQ_ENOMEM;
  else {
    FqDeflateArgs a{d_in, (uint64_t)n, d_stage, d_bs, fqdev::crc_const(), nb, d_out};
    FqDeflatePackArgs pk{d_stage, d_bs, d_off, d_out, nb};
    double ms[FQ_K_COUNT] = {0}; uint64_t ln[FQ_K_COUNT] = {0};
    if (!a.crc || fqdev::h2d(d_in, in, (size_t)n) || (mode == FQ_DEFLATE_DYNAMIC ? fqdev::launch_deflate_dyn(a) : fqdev::launch_deflate(a)) || fqdev::launch_scan(d_bs, d_off, nb) || fqdev::launch_deflate_pack(pk) ||
        fqdev::d2h(&total, d_off + nb, 8) || fqdev::sync()) rc = FQ_ENODEV;
    else if ((int64_t)total > cap) rc = FQ_ELIMIT;
    else if (fqdev::d2h(out, d_out, (size_t)total) || fqdev::sync()) rc = FQ_ENODEV;
    fqdev::time_collect(ms, ln, FQ_K_COUNT);
    if (kernel_ms) *kernel_ms = ms[FQ_K_EMIT];
  }
  for (void *p : {(void *)d_in, (void *)d_stage, (void *)d_out, (void *)d_bs, (void *)d_off}) fqdev::dfree(p);
  *out_len = (int64_t)total;
  return rc;
}
extern "C" int fq_bgzf_deflate_device(int device, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *out_len, double *kernel_ms) {
  return fq_bgzf_deflate_device_mode(device, FQ_DEFLATE_FIXED, in, n, out, cap, out_len, kernel_ms);
}
// (tests) fqd_code_lengths alone, by one wavefront
extern "C" int fq_huffman_lengths_device(int device, const uint32_t *freq, int n_sym, int limit, uint8_t *len_out) {
  if (!freq || !len_out || n_sym < 2 || n_sym > FQD_MAX_SYMS || limit < 1 || limit > 15 || (uint32_t)n_sym > (1u << limit)) return FQ_EINVAL;
  uint64_t sum = 0;
  for (int s = 0; s < n_sym; ++s) sum += freq[s];
  if (sum >> 32) return FQ_EINVAL;
  struct DevScope { fqdev::State *s; ~DevScope() { fqdev::state_destroy(s); } } scope{fqdev::state_create(device)};
  if (!scope.s || fqdev::bind(scope.s)) return FQ_ENODEV;
  uint32_t *d_f = (uint32_t *)fqdev::dmalloc((size_t)n_sym * 4);
  uint8_t *d_l = (uint8_t *)fqdev::dmalloc((size_t)n_sym);
  int rc = FQ_OK;
  if (!d_f || !d_l) rc = FQ_ENOMEM;
  else if (fqdev::h2d(d_f, freq, (size_t)n_sym * 4) || fqdev::launch_code_lengths(d_f, n_sym, limit, d_l) || fqdev::d2h(len_out, d_l, (size_t)n_sym) || fqdev::sync()) rc = FQ_ENODEV;
  fqdev::dfree(d_f); fqdev::dfree(d_l);
  return rc;
}

extern "C" int fq_bam_close(fq_bam_t *b) {
  if (!b) return FQ_EINVAL;
  if (b->sort) {
    const int rc = sort_close(b);
    if (b->zst_at_close) { *b->zst_at_close = b->zst; b->zst_at_close->mode = b->deflate_mode; }
    if (rc) fprintf(stderr, "fq_bam_close: %s\n", b->err.c_str());
    if (b->z.fp) { fclose(b->z.fp); b->z.fp = nullptr; }      // (after a failed close; the runs' files go with the writer)
    delete b;
    return rc;
  }
  b->z.close();
  const bool ok = b->z.ok;
  if (b->zst_at_close) { *b->zst_at_close = b->zst; b->zst_at_close->mode = b->deflate_mode; }
  delete b;
  return ok ? FQ_OK : FQ_EIO;
}
