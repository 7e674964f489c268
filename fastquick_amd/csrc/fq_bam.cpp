// fq_bam.cpp -- the BAM consumer of the alignment records: BwtMapper::SetSamRecord (src/BwtMapper.cpp:977-1264, the BAM_DEBUG
// branches that are compiled in: :946) and SetSamFileHeader (:947-975), written as BAM through an own BGZF layer (zlib raw deflate
// in 64 KB blocks).  Unlike the --sam_out dialect the records carry GENOME coordinates: a reduced-reference contig is named
// CHR:POS@REF/ALT[|L], the record's RNAME is CHR and its position POS - flank + offset-in-contig - 1 (:1026-1043), the header's
// @SQ lines are the original reference's (.fai), and every record carries RG:Z.  The record itself is fq_emit.h's fq_bam_record, the
// routine the consumers' kernels run: the host formatter loops over it on the host's view of the call (fq_ctx_host_view).
#include <zlib.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
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

}  // namespace

struct fq_bam {
  // the formatter's tables (fq_emit.h: FqBamArgs): per contig the BAM reference id of its chromosome and where it lies in the genome;
  // made with the writer, uploaded when the first call formats on the device
  std::vector<int32_t> ctg_rid, ctg_g0;
  std::mutex dev_mu;
  bool dev_on = false;
  bool host_deflate = [] { const char *e = getenv("FASTQUICK_BAM_HOST_DEFLATE"); return e && *e && *e != '0'; }();   // A/B: zlib on the host's threads for device-formatted records too
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

extern "C" int fq_bam_create(const fq_index_t *ix, const char *fai_path, const char *bam_path, const char *rg_line, const fq_qc_opts_t *o, fq_bam_t **out) {
  if (!ix || !fai_path || !o || !out) return FQ_EINVAL;
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

bool fq_bam_wants_members(const fq_bam *b) { return b->z.fp != nullptr && !b->host_deflate; }
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
extern "C" int fq_bam_add_last(fq_bam_t *b, fq_ctx_t *c) {
  if (!b || !c || !b->z.fp) return FQ_EINVAL;
  if (const FqBamCallOut *D = fq_ctx_bam_out(c)) {        // the records were formatted by the call's kernels (fq_ctx_attach_bam): they only leave the device here
    if (D->owner != b || !D->ready) { b->err = "fq_bam_add_last: the context's last call formatted its records for another writer, or failed"; return FQ_EINVAL; }
    if (fq_ctx_emit_wait(c)) { b->err = "fq_bam_add_last: waiting for the call's kernels failed"; return FQ_ENODEV; }      // (z_bytes comes back with them)
    int64_t n;
    if (D->z_bytes) {       // finished BGZF members (fq_deflate.h): appended behind whatever the host's layer still holds
      b->z.flush_all();
      n = fq_ctx_bam_stream(c, [](void *user, const void *data, int64_t len) -> int { ((fq_bam *)user)->z.write_members(data, (size_t)len); return ((fq_bam *)user)->z.ok ? 0 : 1; }, b, 1);
    } else n = fq_ctx_bam_stream(c, [](void *user, const void *data, int64_t len) -> int { ((fq_bam *)user)->z.write(data, (size_t)len); return ((fq_bam *)user)->z.ok ? 0 : 1; }, b, 0);
    if (n < 0) { b->err = "fq_bam_add_last: fetching the records from the device failed"; return (int)n; }
    return b->z.ok ? FQ_OK : FQ_EIO;
  }
  const int rc = format_last(b, c);
  if (rc) return rc;
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
  if (len) b->z.write(data, (size_t)len);
  return b->z.ok ? FQ_OK : FQ_EIO;
}
// (tests, tools) n bytes as BGZF members written by the device's compressor (fq_deflate.h): the members behind each other into out (capacity cap);
// *out_len their size, *kernel_ms the compressor kernel's time.  FQ_ELIMIT when cap is too small.
extern "C" int fq_bgzf_deflate_device(int device, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *out_len, double *kernel_ms) {
  if (!in || !out || !out_len || n < 0) return FQ_EINVAL;
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
    FqDeflateArgs a{d_in, (uint64_t)n, d_stage, d_bs, fqdev::crc_const(), nb};
    FqDeflatePackArgs pk{d_stage, d_bs, d_off, d_out, nb};
    double ms[FQ_K_COUNT] = {0}; uint64_t ln[FQ_K_COUNT] = {0};
    if (!a.crc || fqdev::h2d(d_in, in, (size_t)n) || fqdev::launch_deflate(a) || fqdev::launch_scan(d_bs, d_off, nb) || fqdev::launch_deflate_pack(pk) ||
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

extern "C" int fq_bam_close(fq_bam_t *b) {
  if (!b) return FQ_EINVAL;
  b->z.close();
  const bool ok = b->z.ok;
  delete b;
  return ok ? FQ_OK : FQ_EIO;
}
