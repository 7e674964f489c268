// fq_qc.cpp -- the QC consumer of the alignment records: what StatCollector does with every pair that
// BwtMapper::PairEndMapper hands it (src/BwtMapper.cpp:2047-2050 / 2075-2079) and the files its ProcessCore writes
// (src/StatCollector.cpp:2012-2028).
// What happens to a pair is stated ONCE, in fq_emit.h (AddAlignment :950-1101, AddSingleAlignment :424-620, ProcessPairStatus
// :623-921 as FQ_HD routines), and run by two loops: the kernels of a context the consumer is attached to (fq_ctx_attach_qc), and
// the host loop below (fq_qc::host_call) over the arrays of a call that landed on the host (fq_ctx_host_view).  Both leave the same
// forms -- sums in tables, lines and pileup entries in input order, counters, duplicate keys -- and this file turns them into the
// consumer's state with one piece of code each (fold, take_lines, take_piles, take_keys, add_counts).  What holds the 13 files
// to the reference is the reference's own output (tests/golden, the soak against oracle/_ref), on both loops; the loops agreeing
// with each other would show nothing, they run the same text.
// Restated here from the reference's behaviour, function by function:
//   RestoreVcfSites      src/StatCollector.cpp:1742-1839   marker / dbSNP / GC tables, flank regions
//   GetDepthDist .. SummaryOutput  :1858-2028, 2343-2483   the output files
// Containers whose iteration order reaches an output (.SexChromInfo: an unordered_map walked in bucket order) are the same
// standard containers, filled in the same order, so the files come out byte for byte; the others are order-free sums.
//   GetInsertSizeDist    :1969-2002 + src/InsertSizeEstimator.cpp:43-173   the censoring-adjusted insert-size density
//   GetVCF               :2113-2155, 2185-2275   genotype likelihoods of the marker pileups (float arithmetic as there)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/fastquick_amd.h"
#include "fq_index.h"
#include "fq_kernels.h"
#include "fq_pipeline.h"
#include "fq_pool.h"
#include "fq_backend.h"
#include <mutex>
#include <condition_variable>

namespace {
const int kInsertLimit = 4096;                 // INSERT_SIZE_LIMIT

std::string chrom_key(std::string chr) {       // upper case, a name containing "CHR" loses its first three characters (:1760-1764)
  std::transform(chr.begin(), chr.end(), chr.begin(), ::toupper);
  if (chr.find("CHR") != std::string::npos) chr = chr.substr(3);
  return chr;
}

// RegionList (src/RegionList.cpp): start -> end per chromosome, inclusive
struct Regions {
  std::map<std::string, std::map<int, int>> list;
  uint64_t length = 0;
  void add(const std::string &chr, int start, int end) { list[chrom_key(chr)][start] = end; }
  // Union of the regions of each chromosome (what RegionList::Collapse leaves, src/RegionList.cpp:73-113): one sweep over the
  // regions in order of their start, a region that begins inside or at the end of the current one extends it (regions that merely
  // touch -- end + 1 == next start -- stay apart, as there)
  void collapse() {
    length = 0;
    for (auto &chr : list) {
      std::map<int, int> merged;
      bool open = false;
      int lo = 0, hi = 0;
      for (const auto &reg : chr.second) {
        if (open && reg.first <= hi) { hi = std::max(hi, reg.second); continue; }
        if (open) merged[lo] = hi;
        lo = reg.first; hi = reg.second; open = true;
      }
      if (open) merged[lo] = hi;
      chr.second.swap(merged);
      for (const auto &reg : chr.second) length += (uint64_t)(reg.second - reg.first) + 1;
    }
  }
  bool overlapped(const std::string &chr, int pos) const {   // RegionList::IsOverlapped, :48-66
    auto it = list.find(chr);
    if (it == list.end()) return false;
    auto lo = it->second.lower_bound(pos);
    if (lo != it->second.end() && lo->first <= pos && lo->second >= pos) return true;
    if (lo != it->second.begin()) { --lo; if (lo->first <= pos && lo->second >= pos) return true; }
    return false;
  }
};

struct ContigStatus { int overlapped = 0, fully = 0, pair_overlapped = 0, fully_paired = 0; };

struct FileStat {                               // FileStatCollector, src/StatCollector.h:46-62
  long long NumRead = 0, NumBase = 0, TotalFiltered = 0, BwaUnmapped = 0, TotalMAPQ = 0, TotalRetained = 0;
  std::string f1, f2;
};

}  // namespace

struct fq_qc {
  const fq_index *ix = nullptr;
  fq_qc_opts_t o{};
  std::string err;
  // RestoreVcfSites
  struct Marker { std::string chrom_raw, id, ref, alt, qual, filter, info; int pos = 0; };
  std::vector<Marker> markers;
  std::map<std::string, std::map<int, unsigned>> vcf_table;
  // ... flattened for fq_emit.h's routines (the vectors FqQcGeom points into; restore() ends with flatten()): the host loop reads them where they are,
  // device_setup uploads them
  struct Flat {
    std::vector<int32_t> ctg_chrom, ctg_g0, ctg_reg_lo, chr_reg0, reg_start, reg_end, chr_mk0, mk_pos;
    std::vector<uint32_t> reg_base, mk_idx;
    std::vector<uint8_t> ctg_sex, dbsnp;
  } flat;
  template <class P> FqQcGeom geom_through(P p) const {      // p(vector): where the caller's routines find its elements
    FqQcGeom g;
    g.ctg_chrom = p(flat.ctg_chrom); g.ctg_g0 = p(flat.ctg_g0); g.ctg_reg_lo = p(flat.ctg_reg_lo); g.ctg_sex = p(flat.ctg_sex);
    g.chr_reg0 = p(flat.chr_reg0); g.reg_start = p(flat.reg_start); g.reg_end = p(flat.reg_end); g.reg_base = p(flat.reg_base);
    g.chr_mk0 = p(flat.chr_mk0); g.mk_pos = p(flat.mk_pos); g.mk_idx = p(flat.mk_idx); g.dbsnp = p(flat.dbsnp);
    return g;
  }
  // GC content per position: the reference keeps a hash of every position of every marker's window (a later marker's window writes over an
  // earlier one's where they overlap) and reads it at the positions of the flank regions only (GetDepthDist; a position no window covers
  // reads 0): kept here as one byte per flank-region position, laid out like the depth tables
  std::vector<uint8_t> gc_flat;
  Regions flank;
  uint64_t NumXorY = 0, NumShort = 0, NumLong = 0;
  // statistics
  uint64_t NumPCRDup = 0, NumPairReads = 0, NumBaseMapped = 0, NumCov = 0, NumCov2 = 0, NumCov5 = 0, NumCov10 = 0, total_region_size = 0;
  // Depth tables are dense over the flank regions (PositionTable of the reference: a hash of the positions touched so far, whose
  // members all have depth >= 1 -- so the untouched entries of a dense table are exactly its non-members, and every use is a sum)
  std::map<std::string, std::map<int, std::pair<int, size_t>>> flank_idx;   // chrom -> region start -> (region end, first table index)
  std::vector<uint32_t> depth, q20, q30;
  std::vector<std::string> seq_vec, qual_vec;
  std::vector<std::vector<int>> cycle_vec;
  std::vector<std::vector<unsigned char>> maq_vec;
  std::vector<std::vector<bool>> strand_vec;
  std::vector<size_t> DepthDist = std::vector<size_t>(1024, 0), CycleDist = std::vector<size_t>(512, 0), GCDist = std::vector<size_t>(256, 0),
                      PosNum = std::vector<size_t>(101, 0), EmpRep = std::vector<size_t>(256, 0), misEmpRep = std::vector<size_t>(256, 0),
                      EmpCycle = std::vector<size_t>(256, 0), misEmpCycle = std::vector<size_t>(256, 0), InsertDist = std::vector<size_t>(kInsertLimit, 0);
  std::unordered_set<std::string> dup_table;
  std::unordered_map<std::string, ContigStatus> contig_status;
  std::vector<FileStat> files;
  FileStat cur;
  bool file_open = false;
  // ---- shard consumers (fq_qc_state_reset / _export / fq_qc_merge): what the order-dependent outputs need to be put together again
  bool shard = false;                              // logs below are kept since the last reset
  bool cur_continues = false;                      // the open file was begun before the last reset (its counters here are a part of it)
  std::vector<char> files_continue;                // per closed file of this segment: the same
  std::vector<std::string> contig_order;           // sex-chromosome contigs in the order they were first counted (the file walks an unordered_map)
  std::vector<std::string> dup_log;                // key of every proper pair, in order (the duplicate count needs the keys of all shards)
  std::streamoff table_mark = 0;                   // .InsertSizeTable bytes written before the last reset
  ContigStatus &cs(const std::string &name) {
    auto it = contig_status.find(name);
    if (it == contig_status.end()) { if (shard) contig_order.push_back(name); it = contig_status.emplace(name, ContigStatus()).first; }
    return it->second;
  }
  std::string out_prefix;
  std::ofstream table;
  // ---- the sums in the form fq_emit.h's routines keep them (FqQcArgs): the host loop's between its calls, or what pull() fetched from the device.
  //      fold() adds them to the tables above (fq_qc_write, fq_qc_state_export, fq_qc_state_reset)
  struct Sums {
    std::vector<uint32_t> depth, q20, q30, sex_cnt;
    std::vector<uint64_t> hist, insert, est, sex_first;
    void zero(size_t T, size_t nc) {
      depth.assign(T + 1, 0); q20.assign(T + 1, 0); q30.assign(T + 1, 0); sex_cnt.assign((nc + 1) * 4, 0);
      hist.assign(4 * 256, 0); insert.assign((size_t)kInsertLimit, 0); est.assign(4 * (size_t)kInsertLimit, 0); sex_first.assign(nc + 1, ~0ull);
    }
  } host_sums;                                     // (empty until the first host call)
  void fold(const Sums &s);
  // ... and what a call leaves beside them, from either loop
  void take_lines(const char *text, size_t n) { table.write(text, (std::streamsize)n); }      // .InsertSizeTable lines, in input order
  void take_piles(const FqPileEntry *e, size_t n) {                                           // pileup entries, in input order
    for (; n; --n, ++e) {
      seq_vec[e->k] += (char)e->base; qual_vec[e->k] += (char)e->qual;
      cycle_vec[e->k].push_back(e->cyc); maq_vec[e->k].push_back(e->maq); strand_vec[e->k].push_back(e->strand != 0);
    }
  }
  void take_keys(const uint64_t *keys, int n_surv, bool count_repeats);
  void add_counts(const uint64_t *cnt) {                                                      // FQ_QC_C_*
    cur.BwaUnmapped += (long long)cnt[FQ_QC_C_UNMAPPED];
    cur.TotalRetained += (long long)(cnt[FQ_QC_C_RETAINED1] + 2 * cnt[FQ_QC_C_RETAINED2]);
    cur.TotalMAPQ += (long long)(cnt[FQ_QC_C_FAILED1] + 2 * cnt[FQ_QC_C_FAILED2]);
    NumPairReads += 2 * cnt[FQ_QC_C_PROPER];
    NumPCRDup += 2 * cnt[FQ_QC_C_DUP];
  }
  void host_call(FqQcArgs &a);
  // ---- the consumer's tables on the device: set up by the first call of a context this consumer is attached to (fq_ctx_attach_qc);
  //      the sums stay there until pull() fetches them
  std::mutex dev_mu;
  bool dev_on = false;
  bool device_adds = false, host_adds = false;    // a consumer counts its records on one side only (the duplicate set lives there)
  fqdev::State *dev = nullptr;                     // this object's own streams: pull / reset from any thread
  std::vector<void *> d_bufs;                      // the upload of `flat`
  FqQcGeom geom{};
  size_t table_size = 0, n_contigs = 0;
  uint32_t *d_depth = nullptr, *d_q20 = nullptr, *d_q30 = nullptr, *d_sex_cnt = nullptr;
  uint64_t *d_hist = nullptr, *d_insert = nullptr, *d_sex_first = nullptr, *d_dup = nullptr, *d_est = nullptr;
  // what InsertSizeEstimator would read back from the .InsertSizeTable (counted by the device as the lines were decided): valid while every line of
  // the table came from the device path of THIS consumer (no merged segment, no host-side batch)
  std::vector<uint64_t> est_hist = std::vector<uint64_t>(4 * (size_t)kInsertLimit, 0);
  bool est_valid = true;
  uint64_t dup_cap = 0, ord_next = 0;
  // calls of several contexts that share this consumer may overlap (a stream pipelined over two contexts): their counting steps -- which place
  // the call's pairs in the input's order and may grow the duplicate set -- run one at a time, in the order of the calls' order-dependent parts
  std::mutex gate_mu;
  std::condition_variable gate_cv;
  uint64_t tickets = 0, serving = 0;
  int device_setup();
  int pull();                                      // both loops' sums -> the tables above; theirs start again from zero
  int bind_own();
  ~fq_qc() { if (dev_on || dev) { if (!bind_own()) { for (void *b : d_bufs) fqdev::dfree(b); for (void *b : {(void *)d_depth, (void *)d_q20, (void *)d_q30, (void *)d_sex_cnt, (void *)d_hist, (void *)d_insert, (void *)d_sex_first, (void *)d_dup, (void *)d_est}) fqdev::dfree(b); } if (dev) fqdev::state_destroy(dev); } }

  int restore(const std::string &ref_prefix);
  void flatten(const std::unordered_map<std::string, std::unordered_map<int, unsigned>> &dbsnp);
  FqWorkPool pool;                         // the workers fq_qc_write spreads the markers' lines over
};

int fq_qc::restore(const std::string &ref_prefix) {
  std::ifstream vcf(ref_prefix + ".SelectedSite.vcf"), gcf(ref_prefix + ".gc", std::ios_base::binary), db(ref_prefix + ".dbSNP.subset.vcf");
  if (!vcf.is_open() || !gcf.is_open() || !db.is_open()) { err = "cannot open " + ref_prefix + ".SelectedSite.vcf / .gc / .dbSNP.subset.vcf"; return FQ_EIO; }
  const int chopped = (int)std::floor(o.read_len * 0.65f + 0.5);   // FLANK_EDGE, :28, :1754
  struct GcWin { std::string chr; int start; uint32_t len; size_t at; };
  std::vector<GcWin> gc_win;
  std::vector<uint8_t> gc_bytes;
  std::string line;
  while (std::getline(vcf, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::stringstream ss(line);
    Marker m;
    std::string pos;
    std::getline(ss, m.chrom_raw, '\t'); std::getline(ss, pos, '\t'); std::getline(ss, m.id, '\t'); std::getline(ss, m.ref, '\t');
    std::getline(ss, m.alt, '\t'); std::getline(ss, m.qual, '\t'); std::getline(ss, m.filter, '\t'); std::getline(ss, m.info, '\t');
    m.pos = atoi(pos.c_str());
    markers.push_back(m);
    const std::string chr = chrom_key(m.chrom_raw);
    vcf_table[chr][m.pos] = (unsigned)markers.size() - 1;
    uint32_t glen = 0;
    gcf.read(reinterpret_cast<char *>(&glen), 4);
    const size_t g_at = gc_bytes.size();
    gc_bytes.resize(g_at + glen);
    gcf.read(reinterpret_cast<char *>(gc_bytes.data() + g_at), glen);
    if (!gcf) { err = "short .gc file"; return FQ_EIO; }
    gc_win.push_back(GcWin{chr, m.pos - ((int)glen - 1) / 2, glen, g_at});
    if (chr == "X" || chr == "Y") { ++NumXorY; flank.add(chr, m.pos - o.flank_len + chopped, m.pos + o.flank_len - chopped); }
    else if (!m.id.empty() && m.id.back() == 'L') { ++NumLong; flank.add(chr, m.pos - o.flank_long_len + chopped, m.pos + o.flank_long_len - chopped); }
    else { ++NumShort; flank.add(chr, m.pos - o.flank_len + chopped, m.pos + o.flank_len - chopped); }
    seq_vec.emplace_back(""); qual_vec.emplace_back(""); cycle_vec.emplace_back(0); maq_vec.emplace_back(0); strand_vec.emplace_back(0);
  }
  flank.collapse();
  {
    size_t at = 0;
    for (const auto &kv : flank.list) for (const auto &r : kv.second) { flank_idx[kv.first][r.first] = std::make_pair(r.second, at); at += (size_t)(r.second - r.first) + 1; }
    depth.assign(at, 0); q20.assign(at, 0); q30.assign(at, 0);
    gc_flat.assign(at, 0);
  }
  for (const GcWin &w : gc_win) {           // in marker order: the later window's values stand where two overlap
    auto fc = flank_idx.find(w.chr);
    if (fc == flank_idx.end() || w.len == 0) continue;
    const int64_t lo = w.start, hi = (int64_t)w.start + w.len - 1;
    auto it = fc->second.upper_bound((int)std::min<int64_t>(lo, INT32_MAX));
    if (it != fc->second.begin()) --it;
    for (; it != fc->second.end() && it->first <= hi; ++it) {
      const int64_t a = std::max<int64_t>(lo, it->first), b = std::min<int64_t>(hi, it->second.first);
      if (a > b) continue;
      memcpy(gc_flat.data() + it->second.second + (size_t)(a - it->first), gc_bytes.data() + w.at + (size_t)(a - lo), (size_t)(b - a + 1));
    }
  }
  std::unordered_map<std::string, std::unordered_map<int, unsigned>> dbsnp;
  while (std::getline(db, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::stringstream ss(line);
    std::string c, pos;
    std::getline(ss, c, '\t'); std::getline(ss, pos, '\t');
    dbsnp[chrom_key(c)][atoi(pos.c_str())] = 1;
  }
  flatten(dbsnp);
  return FQ_OK;
}

// RestoreVcfSites' tables as fq_emit.h's routines read them (FqQcGeom): per contig its chromosome, its place in the genome (AddSingleAlignment's
// readRealStart, :424-440; AddMatchBaseInfo's chromosome key, :362-379) and where a read's walk over the flank regions starts; per chromosome its flank
// regions and markers in increasing position; the known variant sites as a flag per flank position
void fq_qc::flatten(const std::unordered_map<std::string, std::unordered_map<int, unsigned>> &dbsnp) {
  const size_t nc = ix->contigs.size();
  n_contigs = nc;
  table_size = depth.size();
  std::vector<std::string> chroms;                  // the chromosomes of the flank regions (the markers' chromosomes: the same keys)
  std::map<std::string, int> chrom_id;
  for (const auto &kv : flank_idx) { chrom_id[kv.first] = (int)chroms.size(); chroms.push_back(kv.first); }
  for (const auto &kv : vcf_table) if (!chrom_id.count(kv.first)) { chrom_id[kv.first] = (int)chroms.size(); chroms.push_back(kv.first); }
  std::vector<int32_t> &ctg_chrom = flat.ctg_chrom, &ctg_g0 = flat.ctg_g0, &ctg_reg_lo = flat.ctg_reg_lo, &chr_reg0 = flat.chr_reg0, &reg_start = flat.reg_start, &reg_end = flat.reg_end,
                       &chr_mk0 = flat.chr_mk0, &mk_pos = flat.mk_pos;
  std::vector<uint32_t> &reg_base = flat.reg_base, &mk_idx = flat.mk_idx;
  std::vector<uint8_t> &ctg_sex = flat.ctg_sex, &db = flat.dbsnp;
  ctg_chrom.assign(nc, 0); ctg_g0.assign(nc, 0); ctg_reg_lo.assign(nc, 0); ctg_sex.assign(nc, 0);
  chr_reg0.assign(chroms.size() + 1, 0); chr_mk0.assign(chroms.size() + 1, 0);
  for (size_t i = 0; i < nc; ++i) {
    const std::string &nm = ix->contigs[i].name;
    ctg_sex[i] = nm.find('Y') != std::string::npos || nm.find('X') != std::string::npos;
    const size_t colon = nm.find(':');
    if (colon == std::string::npos) { ctg_chrom[i] = -2; ctg_g0[i] = 0; continue; }
    const size_t at = nm.find('@');
    const int refCoord = (int)strtol(nm.substr(colon + 1, at - colon + 1).c_str(), nullptr, 10);
    const int fl = nm[nm.size() - 1] == 'L' ? o.flank_long_len : o.flank_len;
    ctg_g0[i] = refCoord - fl;
    auto it = chrom_id.find(chrom_key(nm.substr(0, colon)));
    ctg_chrom[i] = it == chrom_id.end() ? -1 : it->second;
  }
  for (size_t c = 0; c < chroms.size(); ++c) {
    chr_reg0[c] = (int32_t)reg_start.size();
    auto fi = flank_idx.find(chroms[c]);
    if (fi != flank_idx.end()) for (const auto &r : fi->second) { reg_start.push_back(r.first); reg_end.push_back(r.second.first); reg_base.push_back((uint32_t)r.second.second); }
    chr_mk0[c] = (int32_t)mk_pos.size();
    auto vi = vcf_table.find(chroms[c]);
    if (vi != vcf_table.end()) for (const auto &m : vi->second) { mk_pos.push_back(m.first); mk_idx.push_back(m.second); }
  }
  chr_reg0[chroms.size()] = (int32_t)reg_start.size(); chr_mk0[chroms.size()] = (int32_t)mk_pos.size();
  for (size_t i = 0; i < nc; ++i) {          // where a read on contig i starts its walk over the flank regions: the first region of its chromosome that ends at or behind the contig's first base
    if (ctg_chrom[i] < 0) continue;
    const int r0 = chr_reg0[(size_t)ctg_chrom[i]], r1 = chr_reg0[(size_t)ctg_chrom[i] + 1];
    const int first = ctg_g0[i];               // (genome coordinate of offset 0 of the contig; a read's bases lie at or behind it)
    ctg_reg_lo[i] = (int32_t)(std::lower_bound(reg_end.begin() + r0, reg_end.begin() + r1, first) - reg_end.begin());
  }
  db.assign(table_size + 1, 0);
  for (const auto &kv : flank_idx) {                 // the known variant sites that lie in a flank region (the only positions the statistics look at)
    auto di = dbsnp.find(kv.first);
    if (di == dbsnp.end()) continue;
    for (const auto &site : di->second) {
      auto r = kv.second.upper_bound(site.first);
      if (r == kv.second.begin()) continue;
      --r;
      if (site.first >= r->first && site.first <= r->second.first) db[r->second.second + (size_t)(site.first - r->first)] = 1;
    }
  }
}

// ---- the device side ---------------------------------------------------------------------------------------------------------
int fq_qc::bind_own() {
  if (!dev) dev = fqdev::state_create(ix->device);
  if (!dev || fqdev::bind(dev)) { err = std::string("QC consumer: no device state: ") + fqdev::last_error(); return FQ_ENODEV; }
  return FQ_OK;
}
// the geometry uploaded, the sums zeroed.  Runs on the calling context's bound state.
int fq_qc::device_setup() {
  if (dev_on) return FQ_OK;
  const size_t nc = n_contigs;
  bool ok = true;
  auto up = [&](const void *src, size_t bytes) -> void * {
    void *d = fqdev::dmalloc(bytes ? bytes : 16);
    if (!d) { ok = false; return nullptr; }
    d_bufs.push_back(d);
    if (bytes && fqdev::h2d(d, src, bytes)) ok = false;
    return d;
  };
  geom = geom_through([&](const auto &v) { return (decltype(v.data()))up(v.data(), v.size() * sizeof v[0]); });
  auto zeroed = [&](size_t bytes, int fill) -> void * {
    void *d = fqdev::dmalloc(bytes ? bytes : 16);
    if (!d) { ok = false; return nullptr; }
    if (fqdev::dfill(d, fill, bytes ? bytes : 16)) ok = false;
    return d;
  };
  d_depth = (uint32_t *)zeroed((table_size + 1) * 4, 0); d_q20 = (uint32_t *)zeroed((table_size + 1) * 4, 0); d_q30 = (uint32_t *)zeroed((table_size + 1) * 4, 0);
  d_hist = (uint64_t *)zeroed(4 * 256 * 8, 0); d_insert = (uint64_t *)zeroed((size_t)kInsertLimit * 8, 0);
  d_sex_cnt = (uint32_t *)zeroed((nc + 1) * 4 * 4, 0); d_sex_first = (uint64_t *)zeroed((nc + 1) * 8, 0xff);
  d_est = (uint64_t *)zeroed(4 * (size_t)kInsertLimit * 8, 0);
  if (!ok || fqdev::sync()) { err = std::string("QC consumer: staging its tables on the device failed: ") + fqdev::last_error(); return FQ_ENODEV; }
  dev_on = true;
  return FQ_OK;
}
// The consumer's part of a call's kernel arguments, on the calling context's bound state: tables, geometry, where this call's pairs stand in the
// input; the duplicate set is grown to hold the call's pairs (calls on contexts that share a consumer must not overlap: the command line's do not).
int fq_qc_device_prepare(fq_qc *q, FqQcArgs *a, int n_surv) {
  std::lock_guard<std::mutex> lk(q->dev_mu);
  if (q->host_adds) { q->err = "QC consumer: records were added on the host before (fq_qc_add_last without fq_ctx_attach_qc): a consumer counts on one side only"; return FQ_EINVAL; }
  int rc = q->device_setup();
  if (rc) return rc;
  q->device_adds = true;
  if (!q->shard) {
    const uint64_t need = 2 * (q->ord_next + (uint64_t)n_surv) + 1024;
    if (need > q->dup_cap) {
      uint64_t cap = 1 << 16;
      while (cap < 2 * need) cap <<= 1;
      uint64_t *tab = (uint64_t *)fqdev::dmalloc(cap * 8);
      if (!tab) { q->err = "QC consumer: out of device memory for the duplicate set"; return FQ_ENOMEM; }
      if (fqdev::dfill(tab, 0xff, cap * 8) || fqdev::launch_dup_rehash(q->d_dup, q->dup_cap, tab, cap - 1) || fqdev::sync()) { fqdev::dfree(tab); q->err = std::string("QC consumer: growing the duplicate set failed: ") + fqdev::last_error(); return FQ_ENODEV; }
      fqdev::dfree(q->d_dup);
      q->d_dup = tab; q->dup_cap = cap;
    }
  }
  a->g = q->geom;
  a->cal_dup = q->o.cal_dup; a->list_keys = q->shard ? 1 : 0;
  a->ord_base = q->ord_next;
  q->ord_next += (uint64_t)n_surv;
  a->depth = q->d_depth; a->q20 = q->d_q20; a->q30 = q->d_q30; a->hist = q->d_hist; a->insert_dist = q->d_insert;
  a->sex_cnt = q->d_sex_cnt; a->sex_first = q->d_sex_first; a->est_hist = q->d_est;
  a->dup_tab = q->d_dup; a->dup_mask = q->dup_cap ? q->dup_cap - 1 : 0;
  return FQ_OK;
}
uint64_t fq_qc_gate_ticket(fq_qc *q) { std::lock_guard<std::mutex> lk(q->gate_mu); return q->tickets++; }
void fq_qc_gate_enter(fq_qc *q, uint64_t ticket) { std::unique_lock<std::mutex> lk(q->gate_mu); q->gate_cv.wait(lk, [&] { return q->serving == ticket; }); }
void fq_qc_gate_leave(fq_qc *q) { { std::lock_guard<std::mutex> lk(q->gate_mu); ++q->serving; } q->gate_cv.notify_all(); }
// What the two loops have summed since the last pull, added to the consumer's tables; theirs start again from zero.
int fq_qc::pull() {
  std::lock_guard<std::mutex> lk(dev_mu);
  if (!host_sums.depth.empty()) { fold(host_sums); host_sums.zero(table_size, n_contigs); }
  if (!dev_on) return FQ_OK;
  int rc = bind_own();
  if (rc) return rc;
  const size_t T = table_size;
  Sums s;
  s.zero(T, n_contigs);
  if (fqdev::d2h(s.depth.data(), d_depth, (T + 1) * 4) || fqdev::d2h(s.q20.data(), d_q20, (T + 1) * 4) || fqdev::d2h(s.q30.data(), d_q30, (T + 1) * 4) || fqdev::d2h(s.hist.data(), d_hist, s.hist.size() * 8) ||
      fqdev::d2h(s.insert.data(), d_insert, s.insert.size() * 8) || fqdev::d2h(s.est.data(), d_est, s.est.size() * 8) ||  fqdev::d2h(s.sex_cnt.data(), d_sex_cnt, s.sex_cnt.size() * 4) || fqdev::d2h(s.sex_first.data(), d_sex_first, s.sex_first.size() * 8) || fqdev::sync() ||
      fqdev::dzero(d_depth, (T + 1) * 4) || fqdev::dzero(d_q20, (T + 1) * 4) || fqdev::dzero(d_q30, (T + 1) * 4) || fqdev::dzero(d_hist, s.hist.size() * 8) || fqdev::dzero(d_insert, s.insert.size() * 8) || fqdev::dzero(d_est, s.est.size() * 8) ||
      fqdev::dzero(d_sex_cnt, s.sex_cnt.size() * 4) || fqdev::dfill(d_sex_first, 0xff, s.sex_first.size() * 8) || fqdev::sync()) {
    err = std::string("QC consumer: reading its tables back failed: ") + fqdev::last_error();
    return FQ_ENODEV;
  }
  fold(s);
  return FQ_OK;
}
// The table forms of fq_emit.h's routines turned into the consumer's tables.
void fq_qc::fold(const Sums &s) {
  {   // the depth is kept as a difference table and, for Q20 / Q30, as the bases BELOW the threshold per position (fq_qc_base_record): a running sum gives the
      // depth, the depth less those the quality depths
    uint32_t sd = 0;
    for (size_t k = 0; k < table_size; ++k) { sd += s.depth[k]; depth[k] += sd; q20[k] += sd - s.q20[k]; q30[k] += sd - s.q30[k]; }
  }
  for (int v = 0; v < 256; ++v) { EmpRep[v] += s.hist[v]; misEmpRep[v] += s.hist[256 + v]; EmpCycle[v] += s.hist[512 + v]; misEmpCycle[v] += s.hist[768 + v]; }
  for (int v = 0; v < kInsertLimit; ++v) InsertDist[v] += s.insert[v];
  for (size_t v = 0; v < s.est.size(); ++v) est_hist[v] += s.est[v];
  std::vector<std::pair<uint64_t, size_t>> order;     // sex-chromosome contigs in the order of their first count
  for (size_t c = 0; c < n_contigs; ++c) if (s.sex_first[c] != ~0ull) order.emplace_back(s.sex_first[c], c);
  std::sort(order.begin(), order.end());
  for (const auto &oc : order) {
    ContigStatus &st = cs(ix->contigs[oc.second].name);
    const uint32_t *sc = &s.sex_cnt[oc.second * 4];
    st.overlapped += (int)sc[0]; st.fully += (int)sc[1]; st.pair_overlapped += (int)sc[2]; st.fully_paired += (int)sc[3];
  }
}
// The duplicate keys a call listed (outer ends of its proper pairs, ~0: none), in pair order, as the reference spells them: "%d:%d:%d" of contig and both ends
// (ProcessPairStatus, :905-916).  A shard consumer logs them for the merge.  count_repeats: they are looked up in this consumer's own set here (the host
// loop; the kernels look theirs up in the set on the device, and list them only for a shard consumer, whose repeats the merge counts).
void fq_qc::take_keys(const uint64_t *keys, int n_surv, bool count_repeats) {
  char key[64];
  for (int sp = 0; sp < n_surv; ++sp) {
    const uint64_t k = keys[sp];
    if (k == FQ_QC_DUP_EMPTY) continue;
    int contig = 0;
    fq_coor_pac2real(ix, (int64_t)(k >> 32), 1, &contig);      // (a proper pair's outer ends lie inside its contig)
    snprintf(key, sizeof key, "%d:%d:%d", contig, (int)(uint32_t)(k >> 32), (int)(uint32_t)k);
    if (count_repeats && !dup_table.insert(key).second) NumPCRDup += 2;
    if (shard) dup_log.emplace_back(key);
  }
}

// ---- the host loop ------------------------------------------------------------------------------------------------------------------
// fq_emit.h's statement over a call whose arrays are in host memory (a.s: fq_ctx_host_view), in the steps the kernels take (fq_align.cpp: emit_measure, emit_fill):
// the pairs' decisions in input order on one thread, the prefix sums that place lines and pileup entries, then per record -- over ranges of pairs on threads of
// their own -- the line, the pileup entries and the per-base sums (depth tables shared and added to atomically, quality / cycle histograms per thread).  The
// duplicate keys are always listed, and this consumer's set looks them up in pair order.
void fq_qc::host_call(FqQcArgs &a) {
  const int P = a.s.n_surv;
  const size_t N = 2 * (size_t)P;
  Sums &s = host_sums;
  if (s.depth.empty()) s.zero(table_size, n_contigs);
  a.ix.pac = ix->pac.data(); a.ix.l_pac = ix->l_pac;
  a.g = geom_through([](const auto &v) { return v.data(); });
  a.cal_dup = o.cal_dup; a.list_keys = 1;
  a.ord_base = ord_next;
  ord_next += (uint64_t)P;
  a.depth = s.depth.data(); a.q20 = s.q20.data(); a.q30 = s.q30.data(); a.hist = s.hist.data(); a.insert_dist = s.insert.data();
  a.sex_cnt = s.sex_cnt.data(); a.sex_first = s.sex_first.data(); a.est_hist = s.est.data();
  uint64_t cnt[FQ_QC_C_COUNT] = {};
  std::vector<int32_t> added(N + 1);
  std::vector<uint32_t> ist_len((size_t)P + 1), pt_cnt(N + 1);
  std::vector<uint64_t> ist_off((size_t)P + 1), pt_off(N + 1), keys((size_t)P + 1);
  a.counters = cnt; a.dup_key = keys.data(); a.added = added.data();
  a.ist_len = ist_len.data(); a.ist_off = ist_off.data(); a.pt_cnt = pt_cnt.data(); a.pt_off = pt_off.data();
  for (int sp = 0; sp < P; ++sp) fq_qc_pair_thread(a, sp);
  for (int sp = 0; sp < P; ++sp) ist_off[(size_t)sp + 1] = ist_off[sp] + ist_len[sp];
  for (size_t i = 0; i < N; ++i) pt_off[i + 1] = pt_off[i] + pt_cnt[i];
  std::vector<char> text(ist_off[P]);
  std::vector<FqPileEntry> pt(pt_off[N]);
  a.ist_text = text.data(); a.pt = pt.data();
  std::vector<uint32_t> hist((size_t)FQ_HOST_RANGES * 4 * 256, 0);
  fq_host_ranges(P, [&](int t, int lo, int hi) {
    for (int idx = lo; idx < hi; ++idx) {
      if (!(idx & 1)) fq_qc_ist_fill_thread(a, idx >> 1);
      fq_qc_pile_fill_thread(a, idx);
      fq_qc_base_record(a, idx, 0, 1, &hist[(size_t)t * 4 * 256]);
    }
  });
  for (size_t b = 0; b < hist.size(); ++b) s.hist[b % (4 * 256)] += hist[b];
  take_lines(text.data(), text.size());
  take_piles(pt.data(), pt.size());
  take_keys(keys.data(), P, true);
  add_counts(cnt);
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------
extern "C" void fq_qc_default_opts(fq_qc_opts_t *o) {
  memset(o, 0, sizeof *o);
  o->flank_len = 250; o->flank_long_len = 1000; o->read_len = 151; o->cal_dup = 1;   // gap_init_opt, libbwa/bwtaln.c:39-48
}
extern "C" int fq_qc_create(const fq_index_t *ix, const char *ref_prefix, const char *out_prefix, const fq_qc_opts_t *o, fq_qc_t **out) {
  if (!ix || !ref_prefix || !out_prefix || !o || !out) return FQ_EINVAL;
  *out = nullptr;
  fq_qc *q = new fq_qc;
  q->ix = ix; q->o = *o; q->out_prefix = out_prefix;
  const int rc = q->restore(ref_prefix);
  if (rc) { delete q; return rc; }
  q->table.open(q->out_prefix + ".InsertSizeTable");
  if (!q->table.is_open()) { delete q; return FQ_EIO; }
  *out = q;
  return FQ_OK;
}
extern "C" void fq_qc_destroy(fq_qc_t *q) { delete q; }
extern "C" const char *fq_qc_last_error(const fq_qc_t *q) { return q ? q->err.c_str() : "null"; }
extern "C" int fq_qc_begin_file(fq_qc_t *q, const char *fq1, const char *fq2) {
  if (!q || !fq1) return FQ_EINVAL;
  q->cur = FileStat();
  q->cur.f1 = fq1; q->cur.f2 = fq2 ? fq2 : fq1;
  q->file_open = true;
  q->cur_continues = false;
  return FQ_OK;
}
extern "C" int fq_qc_end_file(fq_qc_t *q) {
  if (!q || !q->file_open) return FQ_EINVAL;
  q->files.push_back(q->cur);     // StatCollector::AddFSC
  q->files_continue.push_back(q->cur_continues ? 1 : 0);
  q->file_open = false;
  return FQ_OK;
}

// the consumer loop of PairEndMapper over one batch (src/BwtMapper.cpp:2026-2052): counters, then AddAlignment per surviving pair
extern "C" int fq_qc_add_last(fq_qc_t *q, fq_ctx_t *c) {
  if (!q || !c || !q->file_open) return FQ_EINVAL;
  const FqBatchState *S = fq_ctx_state(c);
  const fq_opts_t *ao = fq_ctx_opts(c);
  q->o.mode = ao->mode;
  FileStat &F = q->cur;
  F.NumBase += fq_ctx_last_bases(c);
  F.NumRead += (ao->single_end ? 1LL : 2LL) * S->n_pairs;
  F.TotalFiltered += S->n_pairs - S->n_surv;
  if (const FqQcCallOut *D = fq_ctx_qc_out(c)) {
    // the call counted on the device (fq_ctx_attach_qc): the sums are in the consumer's device tables; what depends on the order of the
    // records came back laid out in input order and is appended here
    if (D->owner != q || !D->ready) { q->err = "fq_qc_add_last: the context's last call counted for another consumer, or failed"; return FQ_EINVAL; }
    if (fq_ctx_emit_wait(c)) { q->err = std::string("fq_qc_add_last: ") + fq_ctx_last_error(c); return FQ_ENODEV; }      // (the call only enqueued its kernels)
    q->add_counts(D->cnt);
    if (D->ist_bytes && fq_ctx_qc_stream(c, 0, [](void *user, const void *data, int64_t n) -> int { ((fq_qc *)user)->take_lines((const char *)data, (size_t)n); return 0; }, q) < 0) {
      q->err = std::string("fq_qc_add_last: fetching the .InsertSizeTable lines failed: ") + fq_ctx_last_error(c);
      return FQ_ENODEV;
    }
    if (D->n_pile && fq_ctx_qc_stream(c, 1, [](void *user, const void *data, int64_t n) -> int { ((fq_qc *)user)->take_piles((const FqPileEntry *)data, (size_t)n / sizeof(FqPileEntry)); return 0; }, q) < 0) {
      q->err = std::string("fq_qc_add_last: fetching the pileup entries failed: ") + fq_ctx_last_error(c);
      return FQ_ENODEV;
    }
    if (q->shard && D->dup_key) q->take_keys(D->dup_key, D->n_surv, false);
    return FQ_OK;
  }
  if (q->device_adds) { q->err = "fq_qc_add_last: this consumer counts on the device (fq_ctx_attach_qc); a batch of a context without it cannot be mixed in"; return FQ_EINVAL; }
  q->host_adds = true;
  q->est_valid = false;
  FqQcArgs a{};
  if (const int rc = fq_ctx_host_view(c, &a.s)) { q->err = std::string("fq_qc_add_last: ") + fq_ctx_last_error(c); return rc; }      // (result arrays left on the device, no qualities)
  q->host_call(a);
  return FQ_OK;
}

// ProcessCore, :2012-2028
// x + 1.0 + 1.0 + ... (t times), every sum rounded as the loop would round it -- without the loop.  Between two powers of two every x + j (j whole) is a
// multiple of the binade's unit, so those additions are exact and may be done at once; the one addition that crosses into the next binade rounds, and is done
// alone.  (InsertSizeEstimator adds 1.0 per table line to cells that start at 1e-6: tens of millions of dependent additions for a deep run.)
static double add_ones(double x, uint64_t t) {
  while (t) {
    if (!(x >= 1.0) || x >= 4503599627370496.0) { x += 1.0; --t; continue; }      // below 1 (the first addition rounds) or past 2^52 (every one may)
    int e; (void)std::frexp(x, &e);                    // x in [2^(e-1), 2^e)
    const double top = std::ldexp(1.0, e);
    const double room = std::ceil(top - x) - 1.0;      // whole steps that stay below `top` (top - x is exact: same binade)
    const uint64_t j = room < 1.0 ? 0 : (uint64_t)std::min<double>(room, (double)t);
    if (j) { x += (double)j; t -= j; }
    if (t) { x += 1.0; --t; }                          // the crossing
  }
  return x;
}
extern "C" double fq_qc_add_ones(double x, uint64_t t) { return add_ones(x, t); }      // (for the test that holds it to the loop)
namespace {
struct WriteTrace {
  bool on; double t0, t;
  WriteTrace() : on(getenv("FASTQUICK_TRACE") != nullptr), t0(now()), t(t0) {}
  static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return 1e3 * (double)ts.tv_sec + 1e-6 * (double)ts.tv_nsec; }
  void mark(const char *what) { if (!on) return; const double n = now(); fprintf(stderr, "TRACE -   QC files   %8.1f ms  %s\n", n - t, what); t = n; }
};
}  // namespace
extern "C" int fq_qc_write(fq_qc_t *q) {
  if (!q) return FQ_EINVAL;
  WriteTrace wt;
  if (int rc = q->pull()) return rc;
  wt.mark("sums fetched from the device");
  q->table.flush();
  wt.mark(".InsertSizeTable flushed");
  const std::string &pre = q->out_prefix;
  {   // GetDepthDist, :1858-1918
    for (auto &chr : q->flank_idx) {
      for (auto &reg : chr.second)
        for (int pos = reg.first; pos <= reg.second.first; ++pos) {
          const int d = (int)q->depth[reg.second.second + (size_t)(pos - reg.first)];
          if (d == 0) continue;                 // never touched: not in the reference's PositionTable
          q->NumBaseMapped += d;
          ++q->DepthDist[d > 1023 ? 1023 : d];
          const unsigned g = q->gc_flat[reg.second.second + (size_t)(pos - reg.first)];
          q->GCDist[g] += d;
          ++q->PosNum[g];
        }
    }
    for (size_t i = 1; i != q->DepthDist.size(); ++i) {
      q->NumCov += q->DepthDist[i];
      if (i >= 2) q->NumCov2 += q->DepthDist[i];
      if (i >= 5) q->NumCov5 += q->DepthDist[i];
      if (i >= 10) q->NumCov10 += q->DepthDist[i];
    }
    const int chopped = (int)std::floor(q->o.read_len * 0.65f + 0.5);
    q->total_region_size = (uint64_t)(((q->o.flank_len - chopped) * 2 + 1) * (int64_t)q->NumShort + ((q->o.flank_long_len - chopped) * 2 + 1) * (int64_t)q->NumLong +
                                      ((q->o.flank_len - chopped) * 2 + 1) * (int64_t)q->NumXorY);
    std::ofstream f(pre + ".DepthDist");
    q->DepthDist[0] = q->total_region_size - q->NumCov;
    for (uint32_t i = 0; i != q->DepthDist.size(); ++i) f << i << "\t" << q->DepthDist[i] << std::endl;
  }
  {   // GetGCDist, :1920-1937
    std::ofstream f(pre + ".GCDist");
    const double MeanDepth = q->NumBaseMapped / (double)q->NumCov;
    for (uint32_t i = 0; i != 101; ++i) {
      f << i << "\t" << q->GCDist[i] << "\t" << q->PosNum[i] << "\t";
      if (q->PosNum[i] == 0) f << 0; else f << (double(q->GCDist[i]) / q->PosNum[i]) / MeanDepth;
      f << std::endl;
    }
  }
  {   // GetEmpRepDist, :1939-1953
    std::ofstream f(pre + ".EmpRepDist");
    for (uint32_t i = 0; i != q->EmpRep.size(); ++i) {
      f << i << "\t" << q->misEmpRep[i] << "\t" << q->EmpRep[i] << "\t";
      if (q->EmpRep[i] == 0) f << 0; else f << (-10) * log10((double)(q->misEmpRep[i] + 1) / (q->EmpRep[i] + 2));
      f << std::endl;
    }
  }
  {   // GetEmpCycleDist, :1955-1972
    std::ofstream f(pre + ".EmpCycleDist");
    double prevQual = 0;
    for (uint32_t i = 0; i != q->EmpCycle.size(); ++i) {
      const double ph = (-10) * log10((double)(q->misEmpCycle[i] + 1e-6) / (q->EmpCycle[i] + 1e-6));
      f << i + 1 << "\t" << q->misEmpCycle[i] << "\t" << q->EmpCycle[i] << "\t" << (q->misEmpCycle[i] == 0 ? prevQual : ph) << "\t" << q->CycleDist[i] << std::endl;
      if (q->misEmpCycle[i] != 0) prevQual = ph;
    }
  }
  {   // GetInsertSizeDist, :1969-1996: the estimator of src/InsertSizeEstimator.cpp reads the .InsertSizeTable file back, once with the
      // "FwdOnly" pairs left out and once with the "RevOnly" ones (InputInsertSizeTable :43-143), and UpdateWeight (:145-173) turns
      // observed (ObsDist) and censored (MisDist) counts per insert size into a density; the two densities are added.
    const int kLimit = 4096;   // INSERT_LIMIT, InsertSizeEstimator.h
    std::vector<double> fsum(2000, 0.);
    for (int pass = 0; pass < 2; ++pass) {
      const std::string skip = pass == 0 ? "FwdOnly" : "RevOnly";
      std::vector<double> Obs(kLimit, 1e-6), Mis(kLimit, 1e-6);
      int totalPair = 0;
      // every line of the table was decided by the device path, which counted what the reader below would take from it: the same additions of 1.0
      // to the same cells (a cell's value depends on how many there were, not on their order), without reading the table back
      const bool counted = q->est_valid && q->device_adds && !q->shard;
      if (counted) {
        for (int k = 0; k < kLimit; ++k) {
          Obs[k] = add_ones(Obs[k], q->est_hist[k]);
          Mis[k] = add_ones(Mis[k], q->est_hist[(pass == 0 ? 2 : 1) * (size_t)kLimit + k] + q->est_hist[3 * (size_t)kLimit + k]);
          totalPair += (int)(q->est_hist[k] + q->est_hist[(pass == 0 ? 2 : 1) * (size_t)kLimit + k] + q->est_hist[3 * (size_t)kLimit + k]);
        }
      }
      std::ifstream fin(counted ? std::string("/dev/null/none") : pre + ".InsertSizeTable");
      std::string line;
      while (std::getline(fin, line)) {
        std::vector<std::string> v;
        for (size_t start = 0;;) {
          const size_t end = line.find('\t', start);
          v.push_back(line.substr(start, end == std::string::npos ? std::string::npos : end - start));
          if (end == std::string::npos) break;
          start = end + 1;
        }
        if (v.size() < 15) continue;
        int Max = atoi(v[1].c_str()), Max2 = atoi(v[2].c_str()), ObsI = atoi(v[3].c_str());
        const int Flag1 = atoi(v[6].c_str()), Flag2 = atoi(v[11].c_str());
        const std::string &Cigar1 = v[8], &Cigar2 = v[13], &Status = v[14];
        if (Max >= kLimit || Max == -1) Max = kLimit - 1;
        if (Max2 >= kLimit || Max2 == -1) Max2 = kLimit - 1;
        if (ObsI >= kLimit || ObsI == -1) ObsI = kLimit - 1;
        if (Status == "Abnormal" || Status == "LowQual" || Status == "NotPair" || Status == skip) continue;
        else if (Status == "FwdOnly") Mis[Max] += 1.;
        else if (Status == "RevOnly") Mis[Max2] += 1.;
        else if (Status == "PropPair") Obs[ObsI] += 1.;
        else if (Status == "PartialPair") {
          const bool s1 = Cigar1.find('S') != std::string::npos, s2 = Cigar2.find('S') != std::string::npos;
          if (!s1 && s2) Mis[(Flag1 & 16) ? Max2 : Max] += 1.;          // read 1 whole: censored on the side it maps to
          else if (s1 && !s2) Mis[(Flag2 & 16) ? Max2 : Max] += 1.;
          else continue;
        } else continue;   // (the reference exits on an unknown status; its own writer produces none)
        ++totalPair;
      }
      std::vector<double> F(2000, 0.), f(2000, 0.), G(2000, 0.), g(2000, 0.);
      for (int k = 0; k < 2000; ++k) {
        const double m = Mis[k], n = Obs[k];
        if (k != 0) { f[k] = n / (1 - G[k - 1]) * 1 / double(totalPair); F[k] = F[k - 1] + f[k]; }
        else { f[k] = n / double(totalPair); F[k] = f[k]; }
        if (k != 0) { g[k] = m / (1 - F[k]) * 1 / double(totalPair); G[k] = G[k - 1] + g[k]; }
        else { g[k] = m / double(totalPair); G[k] = g[k]; }
      }
      for (int k = 0; k < 2000; ++k) fsum[k] = pass == 0 ? f[k] : (fsum[k] + f[k]);
    }
    std::ofstream f(pre + ".AdjustedInsertSizeDist");
    for (size_t i = 0; i < fsum.size(); ++i) f << i << "\t" << fsum[i] << std::endl;
  }
  wt.mark("depth, GC, cycle tables; insert size estimate");
  {   // GetInsertSizeDist's raw table, :1998-2002
    std::ofstream f(pre + ".RawInsertSizeDist");
    for (uint32_t i = 0; i != q->InsertDist.size(); ++i) f << i << "\t" << q->InsertDist[i] << std::endl;
  }
  {   // GetSexChromInfo, :2004-2015
    std::ofstream f(pre + ".SexChromInfo");
    for (auto &kv : q->contig_status)
      f << kv.first << "\t" << kv.second.overlapped << "\t" << kv.second.fully << "\t" << kv.second.pair_overlapped << "\t" << kv.second.fully_paired << std::endl;
  }
  // the markers in the order the two writers below walk them
  struct Site { const std::string *chrom; int pos; unsigned k; };
  std::vector<Site> sites;
  for (auto &chr : q->vcf_table)
    for (auto &site : chr.second) sites.push_back({&chr.first, (int)site.first, site.second});
  const int WT = (int)std::max<size_t>(1, std::min<size_t>({(size_t)16, (size_t)std::max(1, fq_host_cpus()), sites.size() / 64 + 1}));
  const size_t per_site = (sites.size() + (size_t)WT - 1) / (size_t)WT;
  {   // GetPileup, :2030-2065 (the same bytes; a deep run's file is tens of megabytes of single characters: the markers' lines are put together on several threads,
      // a run of markers each, and written in order)
    FILE *fp = fopen((pre + ".Pileup").c_str(), "wb");
    const int qualoffset = (q->o.mode & FQ_MODE_IL13) ? 64 : 33;
    std::vector<std::string> part((size_t)WT);
    auto work = [&](int t) {
      std::string &ln = part[(size_t)t];
      char num[16];
      const size_t lo = (size_t)t * per_site, hi = std::min(sites.size(), lo + per_site);
      size_t need = 0;
      for (size_t i = lo; i < hi; ++i) need += 48 + q->seq_vec[sites[i].k].size() * 8;
      ln.reserve(need);
      for (size_t i = lo; i < hi; ++i) {
        const unsigned k = sites[i].k;
        if (q->seq_vec[k].empty()) continue;
        ln += *sites[i].chrom; ln += '\t';
        ln += std::to_string(sites[i].pos); ln += "\t.\t";
        ln += std::to_string(q->strand_vec[k].size()); ln += '\t';
        for (uint32_t t2 = 0; t2 != q->strand_vec[k].size(); ++t2) ln += (char)(q->strand_vec[k][t2] ? toupper(q->seq_vec[k][t2]) : tolower(q->seq_vec[k][t2]));
        ln += '\t';
        for (uint32_t t2 = 0; t2 != q->qual_vec[k].size(); ++t2) ln += char(q->qual_vec[k][t2] + qualoffset);
        ln += '\t';
        ln.append((const char *)q->maq_vec[k].data(), q->maq_vec[k].size());
        ln += '\t';
        for (uint32_t t2 = 0; t2 != q->cycle_vec[k].size(); ++t2) {
          int v = q->cycle_vec[k][t2], n = 0;
          if (v < 0) { ln += '-'; v = -v; }
          do { num[n++] = (char)('0' + v % 10); v /= 10; } while (v);
          while (n) ln += num[--n];
          if (t2 != q->cycle_vec[k].size() - 1) ln += ',';
        }
        ln += '\n';
      }
    };
    if (WT == 1) work(0); else q->pool.run(WT, work);
    if (fp) { for (auto &ln : part) if (!ln.empty()) fwrite(ln.data(), 1, ln.size(), fp); fclose(fp); }
  }
  wt.mark(".Pileup");
  {   // SummaryOutput, :2343-2483
    std::ofstream fq(pre + ".FASTQ.csv");
    fq << "FileIndex,PairEnd1,PairEnd2" << std::endl;
    for (size_t i = 0; i != q->files.size(); ++i) {
      for (std::string *s : {&q->files[i].f1, &q->files[i].f2}) { const size_t sl = s->find_last_of("\\/"); if (sl != std::string::npos) s->erase(0, sl + 1); }
      fq << i + 1 << "," << q->files[i].f1 << "," << q->files[i].f2 << "\n";
    }
    fq.close();
    std::ofstream fc(pre + ".Sequence.csv");
    long long total_base = 0, total_reads = 0, total_retained = 0, total_unmapped = 0, total_low = 0;
    fc << "FileIndex,NumOfBases,NumOfReads,NumOfUmappedReads,NumOfLowMAPQReads,NumOfQCPassReads,ReadLength" << std::endl;
    for (size_t i = 0; i != q->files.size(); ++i) {
      const FileStat &F = q->files[i];
      fc << i + 1 << "," << F.NumBase << "," << F.NumRead << "," << F.BwaUnmapped << "," << F.TotalMAPQ << "," << F.TotalRetained << ",";
      fc << ((F.NumRead == 0) ? 0 : (F.NumBase / F.NumRead)) << std::endl;
      total_base += F.NumBase; total_reads += F.NumRead; total_retained += F.TotalRetained; total_unmapped += F.BwaUnmapped; total_low += F.TotalMAPQ;
    }
    const double avgReadLen = std::floor(0.5 + ((total_reads == 0) ? 0 : ((double)total_base / total_reads)));
    fc << "Total," << total_base << "," << total_reads << "," << total_unmapped << "," << total_low << "," << total_retained << ",";
    fc << avgReadLen << std::endl;
    fc.close();
    std::ofstream f(pre + ".Summary");
    f << "Statistics : " << "Value\n";
    const uint64_t ref_genome_size = (uint64_t)q->o.genome_size, ref_N_size = (uint64_t)q->o.genome_n_size;
    const auto report_genome_size = ref_genome_size - ref_N_size;
    const double est = (double)q->NumBaseMapped / avgReadLen * report_genome_size / q->total_region_size;
    f << "Estimated Read Mapping Rate : " << est / total_reads << "\n";
    f << "Estimated Read PCR Duplication Rate : " << q->NumPCRDup / ((double)q->NumPairReads) << "[" << q->NumPCRDup << "/" << (double)q->NumPairReads << "]\n";
    f << "Whole Genome Coverage : " << (double)total_base / ref_genome_size << "[" << total_base << "/" << ref_genome_size << "]\n";
    f << "Expected Read Depth : " << (double)total_base / report_genome_size << "[" << total_base << "/" << report_genome_size << "]\n";
    f << "Estimated Read Depth : ";
    f << ((q->NumCov == 0) ? 0 : q->NumBaseMapped / (double)q->total_region_size) << "[" << q->NumBaseMapped << "/" << q->total_region_size << "]\n";
    f << "Reduced Genome Size : " << q->total_region_size << std::endl;
    f << "Depth 1 or above position fraction : " << q->NumCov / (double)q->total_region_size << std::endl;
    f << "Depth 2 or above position fraction : " << q->NumCov2 / (double)q->total_region_size << std::endl;
    f << "Depth 5 or above position fraction : " << q->NumCov5 / (double)q->total_region_size << std::endl;
    f << "Depth 10 or above position fraction : " << q->NumCov10 / (double)q->total_region_size << std::endl;
    long long s20 = 0, s30 = 0;
    for (uint32_t v : q->q20) s20 += v;
    for (uint32_t v : q->q30) s30 += v;
    f << "Q20 Base Fraction : " << (q->NumBaseMapped == 0 ? 0 : double(s20) / q->NumBaseMapped) << std::endl;
    f << "Q30 Base Fraction : " << (q->NumBaseMapped == 0 ? 0 : double(s30) / q->NumBaseMapped) << std::endl;
    f << "Estimated AvgDepth for Q20 bases : " << double(s20) / q->NumCov << std::endl;
    f << "Estimated AvgDepth for Q30 bases : " << double(s30) / q->NumCov << std::endl;
    auto median_from = [&](size_t lo) -> size_t {
      long long tmp = 0, total = 0;
      for (size_t i = lo; i != q->InsertDist.size(); ++i) total += (long long)q->InsertDist[i];
      for (size_t i = lo; i != q->InsertDist.size(); ++i) { tmp += (long long)q->InsertDist[i]; if (tmp > total / 2) return i; }
      return 0;
    };
    f << "Median Insert Size(>=500bp) : " << median_from(500) << std::endl;
    f << "Median Insert Size(>=300bp) : " << median_from(300) << std::endl;
  }
  {   // GetVCF, :2185-2275 (CalLikelihood :2113-2155).  The arithmetic types are the reference's: float accumulators and priors,
      // pow / the 0.5-minus term in double, every other log10 on a float (std::log10(float)), PHRED = (-10) * log10(x), REV_PHRED =
      // pow(10.0, x / -10.0); the file carries the day it was written in its second line.
    std::ofstream fout(pre + ".vcf");
    std::ofstream &f = fout;
    char day[100] = {0};
    { const time_t now = time(nullptr); strftime(day, sizeof day, "%Y%m%d", localtime(&now)); }
    f << "##fileformat=VCFv4.2\n" << "##fileDate=" << day << "\n" << "##source=VerifyBamID2\n";
    f << "##INFO=<ID=AF,Number=A,Type=Float,Description=\"Allele Frequency, for each ALT allele, in the same order as listed\">\n";
    f << "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n";
    f << "##FORMAT=<ID=GP,Number=1,Type=String,Description=\"Genotype\">\n";
    f << "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Normalized, Phred-scaled likelihoods for genotypes as defined in the VCF specification\">\n";
    f << "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tIntendedSample\n";
    // CalLikelihood's terms per quality value (the pileups keep `char` qualities), evaluated with the reference's types: float seq_error = pow(10.0, q / -10.0);
    // std::log10 of a float expression where the expression is float, of a double where it is double
    struct VcfTerms { float one_minus, third, two_thirds; double half_minus; };     // (0.5 - seq_error / 3 is a double expression: its log10 is added as a double)
    std::vector<VcfTerms> vcf_terms(256);
    for (int v = 0; v < 256; ++v) {
      const char qv = (char)(unsigned char)v;
      float seq_error = pow(10.0, (qv / (-10.0)));
      VcfTerms T;
      T.one_minus = std::log10(1 - seq_error); T.half_minus = std::log10(0.5 - seq_error / 3); T.third = std::log10(seq_error / 3); T.two_thirds = std::log10(2 * seq_error / 3);
      vcf_terms[(size_t)v] = T;
    }
    // (a marker's line depends on its own pileup alone: runs of markers on several threads, each into a stream of its own with the file stream's formatting, written in order)
    std::vector<std::string> part((size_t)WT);
    auto work = [&](int t) {
      std::ostringstream f;
      float alleleFrq = 0.;
      const size_t lo = (size_t)t * per_site, hi = std::min(sites.size(), lo + per_site);
      for (size_t si = lo; si < hi; ++si) {
        const unsigned k = sites[si].k;
        const fq_qc::Marker &m = q->markers[k];
        std::string af;   // value of the INFO key AF
        bool has_af = false;
        for (size_t at = 0; at < m.info.size();) {
          size_t end = m.info.find(';', at);
          if (end == std::string::npos) end = m.info.size();
          if (m.info.compare(at, 3, "AF=") == 0) { af = m.info.substr(at + 3, end - at - 3); has_af = true; break; }
          at = end + 1;
        }
        if (!has_af) continue;
        alleleFrq = (float)atof(af.c_str());
        const std::string &seq = q->seq_vec[k], &qual = q->qual_vec[k];
        if (seq.empty()) continue;
        f << m.chrom_raw << "\t" << m.pos << "\t" << m.id << "\t" << m.ref << "\t" << m.alt << "\t" << m.qual << "\t" << m.filter << "\t";
        f << "AF=" << af << ";AC=" << seq.size() << "\t" << "GT:PL:GP\t";
        const char maj = m.ref[0], mnr = m.alt[0];
        float GL0(0), GL1(0), GL2(0);
        for (uint32_t i = 0; i != seq.size(); ++i) {      // (the four terms depend on the quality value alone: looked up, added in the reference's order)
          const VcfTerms &T = vcf_terms[(unsigned char)qual[i]];
          if (seq[i] == maj) { GL0 += T.one_minus; GL1 += T.half_minus; GL2 += T.third; }
          else if (seq[i] == mnr) { GL0 += T.third; GL1 += T.half_minus; GL2 += T.one_minus; }
          else { GL0 += T.two_thirds; GL1 += T.two_thirds; GL2 += T.two_thirds; }
        }
        float PL[3];
        PL[0] = std::floor(GL0 * (-10) + 0.5); PL[1] = std::floor(GL1 * (-10) + 0.5); PL[2] = std::floor(GL2 * (-10) + 0.5);
        float prior[3], post[3], sum;
        prior[0] = (-10) * std::log10((1 - alleleFrq) * (1 - alleleFrq));
        prior[1] = (-10) * std::log10(2 * alleleFrq * (1 - alleleFrq));
        prior[2] = (-10) * std::log10(alleleFrq * alleleFrq);
        post[0] = prior[0] + PL[0]; post[1] = prior[1] + PL[1]; post[2] = prior[2] + PL[2];
        sum = (-10) * std::log10(pow(10.0, (post[0] / (-10.0))) + pow(10.0, (post[1] / (-10.0))) + pow(10.0, (post[2] / (-10.0))));
        post[0] = std::floor(post[0] - sum + 0.5); post[1] = std::floor(post[1] - sum + 0.5); post[2] = std::floor(post[2] - sum + 0.5);
        const char *gt = post[0] < post[1] ? (post[0] < post[2] ? "0/0:" : "1/1:") : (post[1] < post[2] ? "0/1:" : "1/1:");
        f << gt << PL[0] << "," << PL[1] << "," << PL[2] << ":" << post[0] << "," << post[1] << "," << post[2] << "\n";
      }
      part[(size_t)t] = f.str();
    };
    if (WT == 1) work(0); else q->pool.run(WT, work);
    for (auto &ln : part) fout.write(ln.data(), (std::streamsize)ln.size());
  }
  wt.mark("summaries, .vcf");
  return FQ_OK;
}

// ---- the consumer over several ranks -----------------------------------------------------------------------------------------
// Every rank feeds the records of its shard of the input to a consumer of its own; what those consumers have gathered is put
// together on one of them (fq_qc_merge), in the order of the input, and written there (fq_qc_write).  Most of the state is sums
// (FileStatCollector's counters, src/StatCollector.h:46-62; the depth / quality / cycle / insert-size tables of AddSingleAlignment
// and ProcessPairStatus, src/StatCollector.cpp:424-921): those add.  What depends on the order of the records is kept as a log
// and replayed: the .InsertSizeTable lines and the pileup strings of the markers are appended, the duplicate keys of a shard's
// proper pairs are looked up in the union of all shards seen so far (the count of duplicates among N pairs is N minus the distinct
// keys, whatever the order), and the sex-chromosome contigs are entered in the order they were first counted -- .SexChromInfo walks
// an unordered_map, whose order is that of its insertions.
namespace {
struct Out {
  std::vector<uint8_t> b;
  template <class T> void put(const T &v) { const uint8_t *p = (const uint8_t *)&v; b.insert(b.end(), p, p + sizeof(T)); }
  void bytes(const void *p, size_t n) { put<uint64_t>(n); const uint8_t *q = (const uint8_t *)p; b.insert(b.end(), q, q + n); }
  void str(const std::string &s) { bytes(s.data(), s.size()); }
  template <class T> void vec(const std::vector<T> &v) { bytes(v.data(), v.size() * sizeof(T)); }
};
struct In {
  const uint8_t *p, *end;
  bool ok = true;
  template <class T> T get() { T v{}; if ((size_t)(end - p) < sizeof(T)) { ok = false; return v; } memcpy(&v, p, sizeof(T)); p += sizeof(T); return v; }
  const uint8_t *bytes(size_t *n) { *n = (size_t)get<uint64_t>(); if (!ok || (size_t)(end - p) < *n) { ok = false; *n = 0; return p; } const uint8_t *q = p; p += *n; return q; }
  std::string str() { size_t n; const uint8_t *q = bytes(&n); return std::string((const char *)q, n); }
  template <class T> bool vec(std::vector<T> &v) { size_t n; const uint8_t *q = bytes(&n); if (!ok || n % sizeof(T)) { ok = false; return false; } v.resize(n / sizeof(T)); if (n) memcpy(v.data(), q, n); return true; }
};
const uint64_t kStateMagic = 0x3153435146ull;   // "FQCS1"
void put_file(Out &o, const FileStat &F) { o.put(F.NumRead); o.put(F.NumBase); o.put(F.TotalFiltered); o.put(F.BwaUnmapped); o.put(F.TotalMAPQ); o.put(F.TotalRetained); o.str(F.f1); o.str(F.f2); }
FileStat get_file(In &in) { FileStat F; F.NumRead = in.get<long long>(); F.NumBase = in.get<long long>(); F.TotalFiltered = in.get<long long>(); F.BwaUnmapped = in.get<long long>(); F.TotalMAPQ = in.get<long long>(); F.TotalRetained = in.get<long long>(); F.f1 = in.str(); F.f2 = in.str(); return F; }
void add_file(FileStat &a, const FileStat &b) { a.NumRead += b.NumRead; a.NumBase += b.NumBase; a.TotalFiltered += b.TotalFiltered; a.BwaUnmapped += b.BwaUnmapped; a.TotalMAPQ += b.TotalMAPQ; a.TotalRetained += b.TotalRetained; }
}  // namespace

// the marker pileups as GetPileup prints them (fq_qc_write's .Pileup: the same order of the markers, the same characters), with the entries' mapping and
// base qualities as numbers beside them: what `align --popcon_svd` hands to the contamination estimate in memory
extern "C" int fq_qc_piles(const fq_qc_t *q, fq_qc_pile_fn fn, void *user) {
  if (!q || !fn) return FQ_EINVAL;
  const int qualoffset = (q->o.mode & FQ_MODE_IL13) ? 64 : 33;
  std::string bases, quals;
  for (auto &chr : q->vcf_table)
    for (auto &site : chr.second) {
      const unsigned k = site.second;
      const size_t n = q->seq_vec[k].size();
      if (!n) continue;
      bases.resize(n);
      quals.resize(n);
      for (size_t t = 0; t != n; ++t) {
        bases[t] = (char)(q->strand_vec[k][t] ? toupper(q->seq_vec[k][t]) : tolower(q->seq_vec[k][t]));
        quals[t] = char(q->qual_vec[k][t] + qualoffset);
      }
      if (int rc = fn(user, chr.first.c_str(), (int32_t)site.first, (int64_t)n, bases.data(), quals.data(), q->maq_vec[k].data(), (const int8_t *)q->qual_vec[k].data())) return rc;
    }
  return FQ_OK;
}

extern "C" int fq_qc_state_reset(fq_qc_t *q) {
  if (!q) return FQ_EINVAL;
  if (int rc = q->pull()) return rc;       // (what the device holds is dropped with the rest: pulled into the tables that are cleared below)
  q->shard = true;
  std::fill(q->depth.begin(), q->depth.end(), 0u); std::fill(q->q20.begin(), q->q20.end(), 0u); std::fill(q->q30.begin(), q->q30.end(), 0u);
  for (auto *v : {&q->EmpRep, &q->misEmpRep, &q->EmpCycle, &q->misEmpCycle, &q->InsertDist, &q->CycleDist}) std::fill(v->begin(), v->end(), (size_t)0);
  for (size_t k = 0; k < q->seq_vec.size(); ++k) { q->seq_vec[k].clear(); q->qual_vec[k].clear(); q->cycle_vec[k].clear(); q->maq_vec[k].clear(); q->strand_vec[k].clear(); }
  q->NumPCRDup = q->NumPairReads = 0;
  q->dup_log.clear();
  q->contig_status.clear(); q->contig_order.clear();
  q->files.clear(); q->files_continue.clear();
  if (q->file_open) { const std::string f1 = q->cur.f1, f2 = q->cur.f2; q->cur = FileStat(); q->cur.f1 = f1; q->cur.f2 = f2; q->cur_continues = true; }
  q->table.flush();
  q->table_mark = (std::streamoff)q->table.tellp();
  return FQ_OK;
}

extern "C" int64_t fq_qc_state_export(fq_qc_t *q, void *buf, int64_t cap) {
  if (!q) return FQ_EINVAL;
  if (!q->shard) { q->err = "fq_qc_state_export: not a shard consumer (call fq_qc_state_reset before its first batch)"; return FQ_EINVAL; }
  if (int rc = q->pull()) return rc;
  Out o;
  o.put(kStateMagic);
  o.put<int32_t>(q->o.mode);
  o.put<uint64_t>(q->depth.size());
  {   // depth tables: the touched positions (index, depth, Q20, Q30), or the whole tables when most are
    size_t nz = 0;
    for (uint32_t d : q->depth) nz += d != 0;
    const bool dense = nz * 16 > q->depth.size() * 12;
    o.put<uint8_t>(dense ? 1 : 0);
    if (dense) { o.vec(q->depth); o.vec(q->q20); o.vec(q->q30); }
    else {
      std::vector<uint32_t> sp;
      sp.reserve(nz * 4);
      for (size_t k = 0; k < q->depth.size(); ++k) if (q->depth[k]) { sp.push_back((uint32_t)k); sp.push_back(q->depth[k]); sp.push_back(q->q20[k]); sp.push_back(q->q30[k]); }
      o.vec(sp);
    }
  }
  for (auto *v : {&q->EmpRep, &q->misEmpRep, &q->EmpCycle, &q->misEmpCycle, &q->InsertDist, &q->CycleDist}) o.vec(*v);
  {   // pileups: the markers this shard's reads covered
    uint64_t n = 0;
    for (const auto &sq : q->seq_vec) n += !sq.empty();
    o.put(n);
    for (size_t k = 0; k < q->seq_vec.size(); ++k) {
      if (q->seq_vec[k].empty()) continue;
      o.put<uint32_t>((uint32_t)k);
      o.str(q->seq_vec[k]); o.str(q->qual_vec[k]); o.vec(q->cycle_vec[k]); o.vec(q->maq_vec[k]);
      std::vector<uint8_t> st(q->strand_vec[k].begin(), q->strand_vec[k].end());
      o.vec(st);
    }
  }
  o.put<uint64_t>(q->dup_log.size());
  for (const auto &k : q->dup_log) o.str(k);
  o.put<uint64_t>(q->contig_order.size());
  for (const auto &name : q->contig_order) { const ContigStatus &c = q->contig_status[name]; o.str(name); o.put(c.overlapped); o.put(c.fully); o.put(c.pair_overlapped); o.put(c.fully_paired); }
  o.put<uint64_t>(q->files.size());
  for (size_t i = 0; i < q->files.size(); ++i) { o.put<uint8_t>((uint8_t)q->files_continue[i]); put_file(o, q->files[i]); }
  o.put<uint8_t>(q->file_open ? 1 : 0);
  if (q->file_open) { o.put<uint8_t>(q->cur_continues ? 1 : 0); put_file(o, q->cur); }
  {   // the .InsertSizeTable lines of this segment
    q->table.flush();
    std::ifstream fin(q->out_prefix + ".InsertSizeTable", std::ios_base::binary);
    std::string text;
    if (fin.is_open()) { fin.seekg(q->table_mark); text.assign(std::istreambuf_iterator<char>(fin), std::istreambuf_iterator<char>()); }
    o.str(text);
  }
  if (!buf || cap < (int64_t)o.b.size()) return (int64_t)o.b.size();
  memcpy(buf, o.b.data(), o.b.size());
  return (int64_t)o.b.size();
}

extern "C" int fq_qc_merge(fq_qc_t *q, const void *buf, int64_t len) {
  if (!q || !buf || len < 8) return FQ_EINVAL;
  q->est_valid = false;                    // (a merged segment's lines are only in the table file)
  In in{(const uint8_t *)buf, (const uint8_t *)buf + len};
  if (in.get<uint64_t>() != kStateMagic) { q->err = "fq_qc_merge: not an exported consumer state"; return FQ_EINVAL; }
  q->o.mode = in.get<int32_t>();
  if (in.get<uint64_t>() != q->depth.size()) { q->err = "fq_qc_merge: the state belongs to another marker set"; return FQ_EINVAL; }
  if (in.get<uint8_t>()) {
    std::vector<uint32_t> d, a, b;
    if (!in.vec(d) || !in.vec(a) || !in.vec(b) || d.size() != q->depth.size() || a.size() != d.size() || b.size() != d.size()) { q->err = "fq_qc_merge: truncated state"; return FQ_EINVAL; }
    for (size_t k = 0; k < d.size(); ++k) { q->depth[k] += d[k]; q->q20[k] += a[k]; q->q30[k] += b[k]; }
  } else {
    std::vector<uint32_t> sp;
    if (!in.vec(sp) || sp.size() % 4) { q->err = "fq_qc_merge: truncated state"; return FQ_EINVAL; }
    for (size_t t = 0; t < sp.size(); t += 4) { if (sp[t] >= q->depth.size()) { q->err = "fq_qc_merge: corrupt state"; return FQ_EINVAL; } q->depth[sp[t]] += sp[t + 1]; q->q20[sp[t]] += sp[t + 2]; q->q30[sp[t]] += sp[t + 3]; }
  }
  for (auto *v : {&q->EmpRep, &q->misEmpRep, &q->EmpCycle, &q->misEmpCycle, &q->InsertDist, &q->CycleDist}) {
    std::vector<size_t> w;
    if (!in.vec(w) || w.size() != v->size()) { q->err = "fq_qc_merge: truncated state"; return FQ_EINVAL; }
    for (size_t k = 0; k < w.size(); ++k) (*v)[k] += w[k];
  }
  for (uint64_t n = in.get<uint64_t>(); n > 0 && in.ok; --n) {
    const uint32_t k = in.get<uint32_t>();
    const std::string sq = in.str(), ql = in.str();
    std::vector<int> cyc; std::vector<unsigned char> mq; std::vector<uint8_t> st;
    if (!in.vec(cyc) || !in.vec(mq) || !in.vec(st) || k >= q->seq_vec.size()) { q->err = "fq_qc_merge: corrupt state"; return FQ_EINVAL; }
    q->seq_vec[k] += sq; q->qual_vec[k] += ql;
    q->cycle_vec[k].insert(q->cycle_vec[k].end(), cyc.begin(), cyc.end());
    q->maq_vec[k].insert(q->maq_vec[k].end(), mq.begin(), mq.end());
    for (uint8_t v : st) q->strand_vec[k].push_back(v != 0);
  }
  for (uint64_t n = in.get<uint64_t>(); n > 0 && in.ok; --n) {   // the shard's proper pairs against the keys of everything merged so far
    const std::string key = in.str();
    if (!q->dup_table.insert(key).second) q->NumPCRDup += 2;
    q->NumPairReads += 2;
    if (q->shard) q->dup_log.push_back(key);
  }
  for (uint64_t n = in.get<uint64_t>(); n > 0 && in.ok; --n) {
    const std::string name = in.str();
    ContigStatus &c = q->cs(name);
    c.overlapped += in.get<int>(); c.fully += in.get<int>(); c.pair_overlapped += in.get<int>(); c.fully_paired += in.get<int>();
  }
  for (uint64_t n = in.get<uint64_t>(); n > 0 && in.ok; --n) {
    const bool continues = in.get<uint8_t>() != 0;
    const FileStat F = get_file(in);
    if (continues) {
      if (!q->file_open) { q->err = "fq_qc_merge: the state continues a file that is not open here (fq_qc_begin_file)"; return FQ_EINVAL; }
      add_file(q->cur, F);
      q->files.push_back(q->cur); q->files_continue.push_back(q->cur_continues ? 1 : 0);
      q->file_open = false;
    } else { q->files.push_back(F); q->files_continue.push_back(0); }
  }
  if (in.get<uint8_t>()) {
    const bool continues = in.get<uint8_t>() != 0;
    const FileStat F = get_file(in);
    if (continues) {
      if (!q->file_open) { q->err = "fq_qc_merge: the state continues a file that is not open here (fq_qc_begin_file)"; return FQ_EINVAL; }
      add_file(q->cur, F);
    } else { q->cur = F; q->file_open = true; q->cur_continues = false; }
  }
  const std::string text = in.str();
  if (!in.ok) { q->err = "fq_qc_merge: truncated state"; return FQ_EINVAL; }
  q->table.write(text.data(), (std::streamsize)text.size());
  return FQ_OK;
}
