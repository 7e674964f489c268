// fq_vcf.cpp -- fq_svd_read_panel: the panel of `svd` from one or several VCFs, optionally cut down to the sites of a file, read in chunks of text by the
// statements of fq_vcf.h -- as kernels (opts.reader 1) or as host loops over the same bodies (reader 2, the CPU tier: no device is opened).
//
//   per file     the header (## ..., #CHROM) is read on the host through zlib; the records follow as chunks of opts.chunk_bytes of text
//   a chunk      [the unfinished last line of the chunk before | new text], at least one whole line: a chunk without a line end grows
//     BGZF, reader 1   the members are found on the host, their bytes go up, launch_inflate writes the text in HBM; a member the kernel refuses goes through
//                      the host's decoder, then zlib (as the FASTQ front end's)
//     anything else    zlib inflates on the host (plain, gzip, BGZF under reader 2); reader 1 uploads the text
//   stages       line ends (launch_nl_index) -> fq_vcf_site_line -> launch_scan + fq_vcf_compact_line -> k_vcf_geno / fq_vcf_geno_line
//   merge        on the host over the lines' records, in input order: the order-dependent rules of SVDcalculator::ReadVcf ("Duplicated Marker" against the
//                previously kept marker, the first empty line ends the file, the 2^29 cap, the chrom -> pos allele map); a line with needs_host goes through
//                fq_svd_record (fq_svd_host.h), the serial reader's statement, whose verdicts and messages stand.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include <zlib.h>

#include "fastquick_amd.h"
#include "fq_backend.h"
#include "fq_inflate.h"
#include "fq_svd.h"
#include "fq_svd_host.h"
#include "fq_vcf.h"

namespace {
using namespace fqsvd;

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
const uint64_t kMaxLaunchText = 0xfff00000ull;      // a launch covers fewer than 4 GiB of text

template <class T> struct DBuf {
  T *p = nullptr; size_t cap = 0;
  ~DBuf() { if (p) fqdev::dfree(p); }
  bool ensure(size_t n) {
    if (n <= cap) return true;
    if (p) fqdev::dfree(p);
    cap = n + n / 4 + 64;
    p = (T *)fqdev::dmalloc(cap * sizeof(T));
    if (!p) cap = 0;
    return p != nullptr;
  }
  bool ensure_keep(size_t n, size_t keep) {
    if (n <= cap) return true;
    const size_t nc = n + n / 4 + 64;
    T *q = (T *)fqdev::dmalloc(nc * sizeof(T));
    if (!q) return false;
    if (p && keep && (fqdev::d2d(q, p, keep * sizeof(T)) || fqdev::sync())) { fqdev::dfree(q); return false; }
    if (p) fqdev::dfree(p);
    p = q; cap = nc;
    return true;
  }
};

// size of the BGZF member that starts at h (needs >= 18 bytes), 0 if it is none
size_t member_size(const uint8_t *h, size_t n, size_t *hdr_len) {
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
uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// one input file behind its header
struct Source {
  std::string path;
  bool members = false;          // BGZF whose members the device inflates
  gzFile gz = nullptr;
  FILE *f = nullptr;
  std::vector<uint8_t> cbuf;     // compressed bytes not yet consumed: [cpos, cend)
  size_t cpos = 0, cend = 0;
  bool file_eof = false, eof = false;
  ~Source() { if (gz) gzclose(gz); if (f) fclose(f); }
};

struct Reader {
  fq_svd *p = nullptr;
  bool dev = false;
  RecState S;
  fq_svd_read_stats_t st{};
  // the sites
  bool use_sites = false;
  std::vector<uint64_t> keys;
  std::string names;
  std::vector<uint32_t> name_off;
  std::vector<uint8_t> found;
  DBuf<uint64_t> d_keys; DBuf<char> d_names; DBuf<uint32_t> d_name_off; DBuf<uint8_t> d_found;
  // a chunk: the text on the host (h_valid) and, reader 1, in HBM
  std::vector<uint8_t> h_text;
  bool h_valid = true;
  DBuf<uint8_t> d_text[2];
  int cur = 0;
  size_t n = 0;                  // bytes of text in the chunk
  // per-chunk arrays
  std::vector<uint32_t> nl, keep, kept, needs_host;
  std::vector<uint64_t> off;
  std::vector<FqVcfLine> line;
  std::vector<int8_t> g;
  DBuf<uint32_t> d_nl, d_keep, d_kept, d_needs, d_cnt, d_status;
  DBuf<uint64_t> d_off;
  DBuf<FqVcfLine> d_line;
  DBuf<int8_t> d_g;
  DBuf<uint8_t> d_comp;
  DBuf<FqzMember> d_mem;

  int fail(int rc, const std::string &m) { return p->fail(rc, m); }
  int dev_fail(const char *what) { return p->fail(FQ_ENODEV, std::string("svd reader: ") + what + ": " + fqdev::last_error()); }
};

// ---- the header, through zlib: sample names, and how many bytes and lines of text it takes ----
int read_header(Reader &R, const std::string &path, std::vector<std::string> &samples, size_t *hdr_bytes, int64_t *hdr_lines) {
  gzFile f = gzopen(path.c_str(), "rb");
  if (!f) return R.fail(FQ_EIO, "Failed opening file " + path);
  std::string text;
  std::vector<char> buf(1 << 16);
  size_t at = 0;
  int64_t line_no = 0;
  bool eof = false;
  for (;;) {
    size_t e;
    while ((e = text.find('\n', at)) == std::string::npos && !eof) {
      const int got = gzread(f, buf.data(), (unsigned)buf.size());
      if (got < 0) { int en = 0; const std::string m = gzerror(f, &en); gzclose(f); return R.fail(FQ_EIO, path + ": " + m); }
      if (got == 0) eof = true; else text.append(buf.data(), (size_t)got);
    }
    if (e == std::string::npos) { if (at >= text.size()) break; e = text.size(); }
    const char *ln = text.data() + at;
    size_t n = e - at;
    at = std::min(e + 1, text.size());
    ++line_no;
    if (n && ln[n - 1] == '\r') --n;
    if (n >= 2 && ln[0] == '#' && ln[1] == '#') continue;
    gzclose(f);
    if (n >= 2 && ln[0] == '#' && ln[1] == 'C') {
      header_samples(ln, n, samples);
      if (samples.empty()) return R.fail(FQ_EINVAL, "No individual genotype information exist in the input VCF file " + path);
      *hdr_bytes = at; *hdr_lines = line_no;
      return 0;
    }
    return R.fail(FQ_EINVAL, "Header line is not found : #CHROM... (line " + std::to_string(line_no) + " of " + path + ")");
  }
  gzclose(f);
  return R.fail(FQ_EINVAL, "Header line is not found : #CHROM... (" + path + ")");
}

int open_source(Reader &R, Source &s, const std::string &path) {
  s.path = path;
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return R.fail(FQ_EIO, "Failed opening file " + path);
  uint8_t h[18];
  const size_t got = fread(h, 1, sizeof h, f);
  size_t hdr = 0;
  s.members = R.dev && member_size(h, got, &hdr) != 0;
  if (s.members) { rewind(f); s.f = f; return 0; }
  fclose(f);
  s.gz = gzopen(path.c_str(), "rb");
  if (!s.gz) return R.fail(FQ_EIO, "Failed opening file " + path);
  gzbuffer(s.gz, 1 << 20);
  return 0;
}

// ---- text of the next part of the file behind the chunk's n bytes: about `want` bytes (whole members), at least one byte unless the file has ended ----
int append_gz(Reader &R, Source &s, size_t want) {
  const size_t n0 = R.n;
  size_t have = 0;
  while (have < want) {
    const size_t piece = std::min<size_t>(want - have, (size_t)8 << 20);      // (the buffer grows with what the file gives: a small file costs no large one)
    R.h_text.resize(n0 + have + piece);
    const int got = gzread(s.gz, R.h_text.data() + n0 + have, (unsigned)piece);
    if (got < 0) { int en = 0; const std::string m = gzerror(s.gz, &en); return R.fail(FQ_EIO, s.path + ": " + m); }
    if (got == 0) { s.eof = true; break; }
    have += (size_t)got;
  }
  if (s.eof && n0 + have > 0 && R.h_text[n0 + have - 1] != '\n') { R.h_text.resize(n0 + have + 1); R.h_text[n0 + have] = '\n'; ++have; }      // (a last line without a line end)
  R.h_text.resize(n0 + have);
  R.n = n0 + have;
  R.h_valid = true;
  if (R.dev && have) {
    DBuf<uint8_t> &D = R.d_text[R.cur];
    if (!D.ensure_keep(R.n + 64, n0)) return R.fail(FQ_ENOMEM, "svd reader: out of device memory for the text");
    if (fqdev::h2d(D.p + n0, R.h_text.data() + n0, have) || fqdev::sync()) return R.dev_fail("upload");
  }
  return 0;
}

int append_members(Reader &R, Source &s, size_t want) {
  const size_t n0 = R.n;
  std::vector<FqzMember> mem;
  std::vector<uint8_t> comp;
  size_t text = 0;
  while (text < want && !s.eof) {
    if (s.cend - s.cpos < (1u << 17) && !s.file_eof) {      // (a member is at most 64 KiB)
      if (s.cpos) { memmove(s.cbuf.data(), s.cbuf.data() + s.cpos, s.cend - s.cpos); s.cend -= s.cpos; s.cpos = 0; }
      const size_t piece = (size_t)8 << 20;
      if (s.cbuf.size() < s.cend + piece) s.cbuf.resize(s.cend + piece);
      const size_t got = fread(s.cbuf.data() + s.cend, 1, piece, s.f);
      if (got == 0) { if (ferror(s.f)) return R.fail(FQ_EIO, s.path + ": read error"); s.file_eof = true; }
      s.cend += got;
    }
    if (s.cend == s.cpos) { s.eof = true; break; }
    size_t hdr = 0;
    const uint8_t *h = s.cbuf.data() + s.cpos;
    const size_t sz = member_size(h, s.cend - s.cpos, &hdr);
    if (sz == 0 || sz < hdr + 8) return R.fail(FQ_EIO, s.path + ": not a BGZF member at a member boundary (a bgzip file followed by something else?)");
    if (s.cend - s.cpos < sz) { if (s.file_eof) return R.fail(FQ_EIO, s.path + ": truncated BGZF member at the end of the file"); continue; }
    const uint32_t isize = le32(h + sz - 4);
    if (isize) {
      if ((uint64_t)n0 + text + isize > kMaxLaunchText) break;
      FqzMember m{};
      while (comp.size() & 3) comp.push_back(0);
      m.in_off = comp.size(); m.in_len = (uint32_t)(sz - hdr - 8); m.out_off = (uint32_t)(n0 + text); m.out_len = isize; m.crc = le32(h + sz - 8);
      comp.insert(comp.end(), h + hdr, h + sz - 8);
      mem.push_back(m);
      text += isize;
    }
    s.cpos += sz;
  }
  DBuf<uint8_t> &D = R.d_text[R.cur];
  if (!D.ensure_keep(n0 + text + 64 + 512, n0)) return R.fail(FQ_ENOMEM, "svd reader: out of device memory for the text");
  if (!mem.empty()) {
    comp.resize(comp.size() + 2048, 0);      // (the decoder reads ahead of a member's end)
    if (!R.d_comp.ensure(comp.size()) || !R.d_mem.ensure(mem.size()) || !R.d_status.ensure(mem.size())) return R.fail(FQ_ENOMEM, "svd reader: out of device memory for the members");
    const FqzCrcConst *cc = fqdev::crc_const();
    if (!cc) return R.dev_fail("crc tables");
    if (fqdev::h2d(R.d_comp.p, comp.data(), comp.size()) || fqdev::h2d(R.d_mem.p, mem.data(), mem.size() * sizeof(FqzMember))) return R.dev_fail("upload");
    FqInflateArgs a{};
    a.comp = R.d_comp.p; a.mem = R.d_mem.p; a.n_mem = (int32_t)mem.size(); a.out = D.p; a.status = R.d_status.p; a.crc = cc;
    if (fqdev::launch_inflate(a)) return R.dev_fail("inflate");
    std::vector<uint32_t> status(mem.size());
    if (fqdev::d2h(status.data(), R.d_status.p, status.size() * 4) || fqdev::sync()) return R.dev_fail("inflate");
    // members the kernel refused: the host's decoder, then zlib, whose verdict stands
    std::unique_ptr<fqz::Inflater> fz;
    std::vector<uint8_t> tmp;
    for (size_t k = 0; k < mem.size(); ++k) {
      if (status[k] == FQZ_OK) { ++R.st.members; continue; }
      ++R.st.members_host;
      const FqzMember &m = mem[k];
      const uint8_t *src = comp.data() + m.in_off;
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
      if (!ok) return R.fail(FQ_EIO, s.path + ": corrupt BGZF member (inflate or CRC failed)");
      if (fqdev::h2d(D.p + m.out_off, tmp.data(), m.out_len) || fqdev::sync()) return R.dev_fail("upload");
    }
  }
  R.n = n0 + text;
  R.h_valid = false;
  if (s.eof && R.n > 0) {      // a last line without a line end
    uint8_t last = 0;
    if (fqdev::d2h(&last, D.p + R.n - 1, 1) || fqdev::sync()) return R.dev_fail("download");
    if (last != '\n') { last = '\n'; if (fqdev::h2d(D.p + R.n, &last, 1) || fqdev::sync()) return R.dev_fail("upload"); ++R.n; }
  }
  return 0;
}
int append_text(Reader &R, Source &s, size_t want) {
  if ((uint64_t)R.n + want > kMaxLaunchText) {
    if ((uint64_t)R.n + (1u << 16) > kMaxLaunchText) return R.fail(FQ_ELIMIT, s.path + ": a line of 4 GiB or more");
    want = (size_t)(kMaxLaunchText - R.n);
  }
  const double t0 = now();
  const int rc = s.members ? append_members(R, s, want) : append_gz(R, s, want);
  R.st.t_inflate += now() - t0;
  return rc;
}
// the host's copy of the chunk's text (reader 1 over BGZF members: fetched when a line needs the host)
int host_text(Reader &R) {
  if (R.h_valid) return 0;
  R.h_text.resize(R.n);
  if (R.n && (fqdev::d2h(R.h_text.data(), R.d_text[R.cur].p, R.n) || fqdev::sync())) return R.dev_fail("download");
  R.h_valid = true;
  return 0;
}

// ---- the stages over the lines of text[lo, n) ----
int stage_lines(Reader &R, size_t lo) {
  const double t0 = now();
  R.nl.clear();
  if (!R.dev) {
    const uint8_t *T = R.h_text.data();
    for (size_t at = lo; at < R.n;) {
      const uint8_t *q = (const uint8_t *)memchr(T + at, '\n', R.n - at);
      if (!q) break;
      R.nl.push_back((uint32_t)(q - T));
      at = (size_t)(q - T) + 1;
    }
  } else {
    const size_t base = lo & ~(size_t)15;      // (launch_nl_index: lo < 16 in front of a 16-byte aligned text)
    uint8_t *T = R.d_text[R.cur].p + base;
    const uint32_t n = (uint32_t)(R.n - base);
    size_t cap = n / 64 + 1024;
    for (int round = 0; round < 2; ++round) {
      if (!R.d_nl.ensure(cap) || !R.d_cnt.ensure(4)) return R.fail(FQ_ENOMEM, "svd reader: out of device memory for the line index");
      if (fqdev::launch_nl_index(T, n, (uint32_t)(lo - base), R.d_nl.p, (uint32_t)std::min<size_t>(cap, 0xffffffffu), R.d_cnt.p)) return R.dev_fail("line index");
      uint32_t cnt = 0;
      if (fqdev::d2h(&cnt, R.d_cnt.p, 4) || fqdev::sync()) return R.dev_fail("line index");
      if (cnt <= cap) { R.nl.resize(cnt); break; }
      cap = cnt;
    }
    if (!R.nl.empty() && (fqdev::d2h(R.nl.data(), R.d_nl.p, R.nl.size() * 4) || fqdev::sync())) return R.dev_fail("line index");
    for (auto &x : R.nl) x += (uint32_t)base;      // (positions in the chunk)
  }
  R.st.t_lines += now() - t0;
  return 0;
}

int stage_parse(Reader &R, size_t lo) {
  const uint32_t L = (uint32_t)R.nl.size();
  const int32_t N = R.p->N;
  R.line.resize(L); R.keep.resize(L); R.off.resize((size_t)L + 1);
  FqVcfSiteArgs a{};
  a.n = (uint32_t)R.n; a.lo = (uint32_t)lo; a.n_lines = L; a.use_sites = R.use_sites;
  a.sites.n_keys = (uint32_t)R.keys.size(); a.sites.n_names = (uint32_t)(R.name_off.size() - 1);
  FqVcfGenoArgs ga{};
  ga.n = (uint32_t)R.n; ga.n_sample = N;
  double t0 = now();
  if (!R.dev) {
    a.text = R.h_text.data(); a.nl = R.nl.data(); a.line = R.line.data(); a.keep = R.keep.data();
    a.sites.keys = R.keys.data(); a.sites.names = R.names.data(); a.sites.name_off = R.name_off.data(); a.sites.found = R.found.data();
    for (uint32_t i = 0; i < L; ++i) fq_vcf_site_line(a, i);
    uint64_t run = 0;
    for (uint32_t i = 0; i < L; ++i) { R.off[i] = run; run += R.keep[i]; }
    R.off[L] = run;
    R.kept.assign((size_t)run, 0);
    for (uint32_t i = 0; i < L; ++i) fq_vcf_compact_line(R.keep.data(), R.off.data(), R.kept.data(), i);
    R.st.t_site += now() - t0;
    t0 = now();
    const uint32_t K = (uint32_t)run;
    R.g.assign((size_t)K * N, -1); R.needs_host.assign(K, 0);
    ga.text = a.text; ga.line = R.line.data(); ga.kept = R.kept.data(); ga.n_kept = K; ga.g = R.g.data(); ga.needs_host = R.needs_host.data();
    for (uint32_t k = 0; k < K; ++k) fq_vcf_geno_line(ga, k);
    R.st.t_geno += now() - t0;
    return 0;
  }
  // (the nl array in HBM holds positions relative to the aligned base stage_lines used: upload the chunk's)
  if (!R.d_line.ensure(L) || !R.d_keep.ensure(L) || !R.d_off.ensure((size_t)L + 2) || !R.d_kept.ensure(L) || !R.d_nl.ensure(L)) return R.fail(FQ_ENOMEM, "svd reader: out of device memory for the lines");
  if (fqdev::h2d(R.d_nl.p, R.nl.data(), (size_t)L * 4)) return R.dev_fail("upload");
  a.text = R.d_text[R.cur].p; a.nl = R.d_nl.p; a.line = R.d_line.p; a.keep = R.d_keep.p;
  a.sites.keys = R.d_keys.p; a.sites.names = R.d_names.p; a.sites.name_off = R.d_name_off.p; a.sites.found = R.d_found.p;
  if (fqdev::launch_vcf_site(a) || fqdev::launch_scan(R.d_keep.p, R.d_off.p, L) || fqdev::launch_vcf_compact(R.d_keep.p, R.d_off.p, R.d_kept.p, L)) return R.dev_fail("site kernel");
  uint64_t run = 0;
  if (fqdev::d2h(&run, R.d_off.p + L, 8) || fqdev::d2h(R.line.data(), R.d_line.p, (size_t)L * sizeof(FqVcfLine)) || fqdev::sync()) return R.dev_fail("site kernel");
  R.st.t_site += now() - t0;
  t0 = now();
  const uint32_t K = (uint32_t)run;
  if (K > L) return R.fail(FQ_ENODEV, "svd reader: the compaction kept more lines than there are");
  R.kept.resize(K); R.g.resize((size_t)K * N); R.needs_host.resize(K);
  if (K) {
    if (!R.d_g.ensure((size_t)K * N) || !R.d_needs.ensure(K)) return R.fail(FQ_ENOMEM, "svd reader: out of device memory for the genotypes");
    if (fqdev::dfill(R.d_g.p, 0xff, (size_t)K * N) || fqdev::dzero(R.d_needs.p, (size_t)K * 4)) return R.dev_fail("genotype kernel");
    ga.text = a.text; ga.line = R.d_line.p; ga.kept = R.d_kept.p; ga.n_kept = K; ga.g = R.d_g.p; ga.needs_host = R.d_needs.p;
    if (fqdev::launch_vcf_geno(ga)) return R.dev_fail("genotype kernel");
    if (fqdev::d2h(R.kept.data(), R.d_kept.p, (size_t)K * 4) || fqdev::d2h(R.g.data(), R.d_g.p, (size_t)K * N) || fqdev::d2h(R.needs_host.data(), R.d_needs.p, (size_t)K * 4) || fqdev::sync())
      return R.dev_fail("genotype kernel");
  }
  R.st.t_geno += now() - t0;
  return 0;
}

// the order-dependent rules, line by line.  *stop: an empty line ended the file
int merge(Reader &R, bool *stop) {
  const double t0 = now();
  fq_svd *p = R.p;
  const uint32_t L = (uint32_t)R.line.size();
  uint32_t k = 0;      // the next kept row
  std::string chrom;
  for (uint32_t i = 0; i < L; ++i) {
    const FqVcfLine &ln = R.line[i];
    ++R.S.line_no;
    ++R.st.lines;
    const bool geno = (ln.flags & FQV_F_GENO) != 0;
    const uint32_t row = geno ? k++ : 0;
    if (!(ln.flags & FQV_F_SITE)) continue;      // not a site's record: as if it were not in the file
    ++R.st.site_lines;
    if (ln.flags & FQV_F_EMPTY) { *stop = true; break; }
    const bool errs = (ln.flags & FQV_F_LT5) || ((ln.flags & FQV_F_CHROM_OK) && !(ln.flags & FQV_F_INDEL) && (ln.flags & (FQV_F_NOALLELE | FQV_F_LT10 | FQV_F_NOKEY)));
    if ((ln.flags & FQV_F_HOST) || errs || (geno && R.needs_host[row])) {
      if (int rc = host_text(R)) return rc;
      ++R.st.host_lines;
      const int rc = fq_svd_record(p, R.S, (const char *)R.h_text.data() + ln.beg, ln.len);
      if (rc < 0) return rc;
      continue;
    }
    if (!(ln.flags & FQV_F_LONGCHROM)) {
      chrom.assign(ln.chrom, ln.chrom_len);
      if (R.S.have_prev && R.S.prev_pos == ln.pos && R.S.prev_chrom == chrom) return p->fail(FQ_EINVAL, "Duplicated Marker at " + chrom + ":" + std::to_string(ln.pos) + R.S.where());
    }
    if (!geno) continue;      // another chromosome, or an indel
    if (fq_svd_install(p, R.S, chrom, ln.pos, ln.ref, ln.alt, R.g.data() + (size_t)row * p->N) < 0) return FQ_ELIMIT;
  }
  R.st.t_host += now() - t0;
  return 0;
}

int read_file(Reader &R, const std::string &path, size_t hdr_bytes, int64_t hdr_lines) {
  Source s;
  if (int rc = open_source(R, s, path)) return rc;
  R.S.path = path;
  R.S.line_no = hdr_lines;
  R.n = 0; R.h_text.clear(); R.h_valid = true;
  size_t skip = hdr_bytes;
  const size_t chunk = (size_t)std::min<int64_t>(std::max<int64_t>(R.p->o.chunk_bytes, 1), (int64_t)1 << 31);
  bool stop = false;
  while (!stop) {
    // the chunk: at least one whole line behind the header's bytes
    bool grown = false;
    for (;;) {
      if (!s.eof && (R.n < chunk + skip || grown)) { if (int rc = append_text(R, s, std::max(chunk + skip > R.n ? chunk + skip - R.n : 0, grown ? chunk : (size_t)1))) return rc; }
      if (skip >= R.n) { if (s.eof) return 0; skip -= R.n; R.n = 0; R.h_text.clear(); grown = false; continue; }      // (all header so far)
      if (int rc = stage_lines(R, skip)) return rc;
      if (!R.nl.empty() || s.eof) break;
      grown = true;
    }
    if (R.nl.empty()) return 0;      // (the file has ended: its last line got a line end, so nothing is left)
    ++R.st.chunks;
    if (int rc = stage_parse(R, skip)) return rc;
    if (int rc = merge(R, &stop)) return rc;
    // what is behind the last line end leads the next chunk
    const size_t used = (size_t)R.nl.back() + 1, rest = R.n - used;
    if (stop || (rest == 0 && s.eof)) return 0;
    if (R.dev) {
      DBuf<uint8_t> &D = R.d_text[R.cur ^ 1];
      if (!D.ensure(rest + chunk + 64 + 512)) return R.fail(FQ_ENOMEM, "svd reader: out of device memory for the text");
      if (rest && (fqdev::d2d(D.p, R.d_text[R.cur].p + used, rest) || fqdev::sync())) return R.dev_fail("carry");
      R.cur ^= 1;
    }
    if (R.h_valid) { R.h_text.erase(R.h_text.begin(), R.h_text.begin() + (ptrdiff_t)used); }
    else R.h_text.clear();
    R.n = rest;
    skip = 0;
  }
  return 0;
}

int read_sites(Reader &R, const char *path) {
  gzFile f = gzopen(path, "rb");
  if (!f) return R.fail(FQ_EIO, std::string("Failed opening file ") + path);
  std::string text;
  std::vector<char> buf(1 << 20);
  for (;;) {
    const int got = gzread(f, buf.data(), (unsigned)buf.size());
    if (got < 0) { int en = 0; const std::string m = gzerror(f, &en); gzclose(f); return R.fail(FQ_EIO, std::string(path) + ": " + m); }
    if (got == 0) break;
    text.append(buf.data(), (size_t)got);
  }
  gzclose(f);
  std::map<std::string, uint32_t> ord;
  std::vector<std::string> order;
  int64_t line_no = 0;
  for (size_t at = 0; at < text.size();) {
    size_t e = text.find('\n', at);
    if (e == std::string::npos) e = text.size();
    const char *ln = text.data() + at;
    size_t n = e - at;
    at = e + 1;
    ++line_no;
    if (n && ln[n - 1] == '\r') --n;
    if (n == 0 || ln[0] == '#') continue;
    const char *t1 = (const char *)memchr(ln, '\t', n);
    if (!t1) return R.fail(FQ_EINVAL, "--Sites: a line without CHROM and POS columns (line " + std::to_string(line_no) + " of " + path + ")");
    std::string chrom(ln, (size_t)(t1 - ln));
    if (chrom.size() >= 3 && (!chrom.compare(0, 3, "chr") || !chrom.compare(0, 3, "CHR"))) chrom.erase(0, 3);
    const char *t2 = (const char *)memchr(t1 + 1, '\t', n - (size_t)(t1 + 1 - ln));
    const int32_t pos = atoi(std::string(t1 + 1, t2 ? (size_t)(t2 - t1 - 1) : n - (size_t)(t1 + 1 - ln)).c_str());
    auto it = ord.find(chrom);
    if (it == ord.end()) { it = ord.emplace(chrom, (uint32_t)order.size()).first; order.push_back(chrom); }
    R.keys.push_back((uint64_t)it->second << 32 | (uint32_t)pos);
  }
  std::sort(R.keys.begin(), R.keys.end());
  R.keys.erase(std::unique(R.keys.begin(), R.keys.end()), R.keys.end());
  if (R.keys.size() > 0x7fffffffu) return R.fail(FQ_ELIMIT, "--Sites: more than 2^31 sites");
  R.name_off.assign(1, 0);
  for (const auto &c : order) { R.names += c; R.name_off.push_back((uint32_t)R.names.size()); }
  R.found.assign(R.keys.size() + 1, 0);
  R.use_sites = true;
  return 0;
}

int run(Reader &R, const char *const *paths, int32_t n_paths, const char *sites) {
  fq_svd *p = R.p;
  R.name_off.assign(1, 0);
  R.found.assign(1, 0);
  if (sites) { if (int rc = read_sites(R, sites)) return rc; }
  if (R.dev) {
    if (!p->dev) {
      p->dev = fqdev::state_create(p->o.device);
      if (!p->dev) return R.fail(FQ_ENODEV, std::string("svd: no device for the reader's kernels (") + fqdev::last_error() + "); reader 2 runs the host loops");
    }
    if (fqdev::bind(p->dev)) return R.fail(FQ_ENODEV, fqdev::last_error());
    if (!R.d_keys.ensure(R.keys.size() + 1) || !R.d_names.ensure(R.names.size() + 1) || !R.d_name_off.ensure(R.name_off.size()) || !R.d_found.ensure(R.found.size())) return R.fail(FQ_ENOMEM, "svd reader: out of device memory for the sites");
    if (fqdev::h2d(R.d_keys.p, R.keys.data(), R.keys.size() * 8) || fqdev::h2d(R.d_names.p, R.names.data(), R.names.size()) || fqdev::h2d(R.d_name_off.p, R.name_off.data(), R.name_off.size() * 4) ||
        fqdev::dzero(R.d_found.p, R.found.size()) || fqdev::sync())
      return R.dev_fail("upload of the sites");
  }
  for (int32_t k = 0; k < n_paths; ++k) {
    std::vector<std::string> samples;
    size_t hdr_bytes = 0;
    int64_t hdr_lines = 0;
    if (int rc = read_header(R, paths[k], samples, &hdr_bytes, &hdr_lines)) return rc;
    if (k == 0) { p->samples = samples; p->N = (int32_t)samples.size(); }
    else {
      for (size_t j = 0; j < std::max(samples.size(), p->samples.size()); ++j)
        if (j >= samples.size() || j >= p->samples.size() || samples[j] != p->samples[j])
          return R.fail(FQ_EINVAL, std::string("svd: the sample names of ") + paths[k] + " differ from those of " + paths[0] + " at sample column " + std::to_string(j + 1) + " ('" +
                                       (j < samples.size() ? samples[j] : std::string("")) + "' against '" + (j < p->samples.size() ? p->samples[j] : std::string("")) + "')");
    }
    if (int rc = read_file(R, paths[k], hdr_bytes, hdr_lines)) return rc;
  }
  if (R.dev && R.use_sites && (fqdev::d2h(R.found.data(), R.d_found.p, R.found.size()) || fqdev::sync())) return R.dev_fail("download of the sites");
  R.st.kept = p->M;
  R.st.sites = (int64_t)R.keys.size();
  for (size_t i = 0; i < R.keys.size(); ++i) R.st.sites_found += R.found[i] != 0;
  return 0;
}

}  // namespace

extern "C" int fq_svd_read_panel(fq_svd_t *p, const char *const *paths, int32_t n_paths, const char *sites_or_null) {
  if (!p || !paths || n_paths < 1) return FQ_EINVAL;
  for (int32_t k = 0; k < n_paths; ++k) if (!paths[k]) return FQ_EINVAL;
  if (p->o.reader == 0) {
    if (n_paths != 1 || sites_or_null) return p->fail(FQ_EINVAL, "svd: the serial reader takes one VCF and no sites (reader 1 or 2 reads a list and --Sites)");
    return fq_svd_read_vcf(p, paths[0]);
  }
  // (an empty panel first, by what fq_svd_set_genotypes does: the device arrays of a decomposition go, the stats are zero)
  if (p->dd) { if (p->dev && !fqdev::bind(p->dev)) fqdev::svd_free(p->dd); p->dd = nullptr; }
  auto clear = [&]() {
    p->M = p->N = 0;
    p->g.clear(); p->samples.clear(); p->chrom.clear(); p->pos.clear(); p->bed.clear(); p->gt.clear(); p->c.clear();
    p->ran = false;
  };
  clear();
  p->rs = fq_svd_read_stats_t{};
  const double t0 = now();
  int rc;
  fq_svd_read_stats_t st{};
  {
    Reader R;
    R.p = p;
    R.dev = p->o.reader == 1;
    rc = run(R, paths, n_paths, sites_or_null);
    st = R.st;
  }      // (the reader's device buffers are freed here, the state still bound)
  if (rc) { const std::string m = p->err; clear(); return p->fail(rc, m); }
  p->t_read = now() - t0;
  p->rs = st;
  if (p->N < FQ_SVD_NPC || p->M < FQ_SVD_NPC) {
    char m[200];
    snprintf(m, sizeof m, "svd: %d markers kept and %d samples: the SVD files hold ten components, at least ten of each are needed", p->M, p->N);
    clear();
    return p->fail(FQ_EINVAL, m);
  }
  return 0;
}
