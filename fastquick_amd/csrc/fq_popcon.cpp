// fq_popcon.cpp -- `FASTQuick pop+con` (VerifyBamID2's ContaminationEstimator) around the likelihood of fq_popcon.h.
//
// Host side of the estimate: the readers of .UD / .mu / .bed / --KnownAF files and of a pileup (ContaminationEstimator.cpp:292-438,
// SimplePileupViewer.cpp:767-846, with their stream extraction and its quirks), IsSanityCheckOK (:493-536), the AmoebaMinimizer of
// MathGenMin.cpp:310-443 as plain C++ (the same sequence of evaluated points), the model sequence of OptimizeLLK / FullLLKFunc::Evaluate
// (ContaminationEstimator.cpp:29-282, .h:283-407) and the writers (vb2Main.cpp:249-274, ContaminationEstimator.cpp:104-138).
// The evaluator behind the minimiser is a switch: the kernels of fq_popcon.h (fq_device.hip: pc_llk), or -- opts.host_eval -- the host loop over
// the same statement, which is the CPU tier and the yardstick: it reproduces the reference's doubles bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "fastquick_amd.h"
#include "fq_backend.h"
#include "fq_popcon.h"

namespace {

thread_local std::string g_create_err;

struct Pile { std::vector<char> base, qual; };

// AmoebaMinimizer (MathGenMin.cpp:310-443) over std::vector: Reset's identity directions of scale 1, cycleMax 50000, ZEPS 3e-10, FPMAX 1e100
struct Amoeba {
  typedef std::vector<double> Vec;
  std::function<double(const Vec &)> f;
  std::function<void(const std::vector<Vec> &)> prefetch;   // points whose values will be asked for next, in that order (a batched launch)
  Vec point;
  double fmin = 1.0e+100;
  int cycleCount = 0, cycleMax = 50000;
  std::vector<Vec> simplex;
  Vec y, psum, ptry;
  int dim = 0;
  void reset(int n) {
    dim = n;
    point.assign(n, 0.);
    fmin = 1.0e+100;
    simplex.assign(n + 1, Vec(n, 0.));
    y.assign(n + 1, 0.);
    psum.assign(n, 0.);
    ptry.assign(n, 0.);
  }
  void sum_simplex() {
    psum = simplex[0];
    for (int m = 1; m < dim + 1; m++) for (int k = 0; k < dim; k++) psum[k] += simplex[m][k];
  }
  double amoeba(int ihi, double factor) {
    const double fac = (1.0 - factor) / dim;
    for (int k = 0; k < dim; k++) ptry[k] = fac * psum[k];
    const double k2 = factor - fac;
    for (int k = 0; k < dim; k++) ptry[k] += k2 * simplex[ihi][k];
    const double ytry = f(ptry);
    if (ytry < y[ihi]) {
      y[ihi] = ytry;
      for (int k = 0; k < dim; k++) psum[k] -= simplex[ihi][k];
      simplex[ihi] = ptry;
      for (int k = 0; k < dim; k++) psum[k] += simplex[ihi][k];
    }
    return ytry;
  }
  double minimize(double ftol, bool *failed) {
    int i, ilo, ihi, inhi;
    const int nvertex = dim + 1;
    double rtol, ysave, ytry;
    if (dim == 0) return fmin = f(point);
    for (i = 0; i < dim; i++) { simplex[i] = point; simplex[i][i] += 1.0; }
    simplex[nvertex - 1] = point;
    if (prefetch) prefetch(simplex);
    for (i = 0; i < nvertex; i++) {
      y[i] = f(simplex[i]);
      if (y[i] < fmin) fmin = y[i];
    }
    cycleCount = nvertex;
    sum_simplex();
    while (true) {
      ihi = y[0] > y[1] ? (ilo = inhi = 1, 0) : (ilo = inhi = 0, 1);
      for (i = 2; i < nvertex; i++) {
        if (y[i] <= y[ilo]) ilo = i;
        else if (y[i] > y[ihi]) { inhi = ihi; ihi = i; }
        else if (y[i] > y[inhi]) inhi = i;
      }
      rtol = 2 * fabs(y[ihi] - y[ilo]) / (fabs(y[ihi]) + fabs(y[ilo]) + 3.0e-10);
      if (rtol < ftol) { point = simplex[ilo]; return fmin = y[ilo]; }
      if (cycleCount > cycleMax) {
        fprintf(stderr, "WARNING - Amoeba.Minimize - Couldn't converge in %d cycles\n", cycleMax);
        *failed = true;
        return std::numeric_limits<double>::max();
      }
      cycleCount += 2;
      ytry = amoeba(ihi, -1.0);
      if (ytry <= y[ilo]) amoeba(ihi, 2.0);
      else if (ytry >= y[inhi]) {
        ysave = y[ihi];
        ytry = amoeba(ihi, 0.5);
        if (ytry >= ysave) {
          std::vector<Vec> ask;
          for (i = 0; i < nvertex; i++)
            if (i != ilo) {
              for (int k = 0; k < dim; k++) simplex[i][k] += simplex[ilo][k];
              for (int k = 0; k < dim; k++) simplex[i][k] *= 0.5;
              ask.push_back(simplex[i]);
            }
          if (prefetch) prefetch(ask);
          for (i = 0; i < nvertex; i++)
            if (i != ilo) y[i] = f(simplex[i]);
          cycleCount += dim;
          sum_simplex();
        }
      } else cycleCount--;
    }
  }
};

}  // namespace

struct fq_popcon {
  fq_popcon_opts_t o{};
  std::string known_af_path, err;
  int numPC = 0;
  uint32_t NumMarker = 0;
  std::vector<std::vector<double>> UD;
  std::vector<double> means;
  std::vector<std::pair<std::string, int>> PosVec;
  std::unordered_map<std::string, std::unordered_map<int, std::pair<char, char>>> ChooseBed;
  std::unordered_map<std::string, std::unordered_map<uint32_t, double>> knownAF;
  std::unordered_map<std::string, std::unordered_map<int, int32_t>> row_of;   // site -> its first row among the NumMarker rows (fq_popcon_marker_index)
  // the viewer (SimplePileupViewer's public fields)
  std::unordered_map<std::string, std::unordered_map<int32_t, int32_t>> posIndex;
  std::vector<Pile> piles;
  int64_t numBases = 0;   // (an int in the reference: a pileup of 2^31 bases is beyond what it reads)
  int effectiveNumSite = 0;
  double avgDepth = 0, sdDepth = 0;
  bool have_pileup = false, sanity_done = false, sanity_failed = false, isPileupInput = false;
  // the estimator's model state (ContaminationEstimator + FullLLKFunc)
  bool isPCFixed = false, isAlphaFixed = false, isAFknown = false, isHeter = true;
  std::vector<double> PC[2];
  double alpha = 0.5;
  double llk1 = 0, llk0 = 0, fixAlpha = 0, globalAlpha = 0;
  std::vector<double> fixPC, fixPC2, globalPC, globalPC2;
  int64_t n_eval = 0;
  bool ran = false;
  // the packed pileup (fq_popcon.h) on the host, and on the device
  bool packed = false;
  std::vector<uint32_t> depth;
  std::vector<uint64_t> off;
  std::vector<uint8_t> code, skip;
  std::vector<double> ud_flat, af_flat;
  std::vector<char> alt;
  int8_t q_of_slot[FQ_PC_MAXQ] = {};
  uint8_t slot_of_q[256] = {};
  int n_q = 0, markers_used = 0;
  FqPcPile hp{};
  fqdev::State *dev = nullptr;
  fqdev::PcDev *pd = nullptr;
  int pd_points = 0;
  std::vector<std::pair<std::vector<double>, double>> cache;   // prefetched values, by the point's bits

  int fail(int rc, const std::string &m) { err = m; return rc; }
};

namespace {

const int kBatch = 2 * FQ_PC_MAXPC + 3;   // the largest simplex (2 * num_pc + 1 dimensions) has one fewer vertices; Initialize's point travels with the first

int read_bed(fq_popcon *p, const std::string &path) {   // ReadChooseBed
  std::ifstream fin(path);
  if (!fin.is_open()) return p->fail(FQ_EIO, "Open file:" + path + "\t failed");
  std::string line, chr;
  int pos(0);
  char ref(0), alt(0);
  while (std::getline(fin, line)) {
    std::stringstream ss(line);
    ss >> chr >> pos >> pos;
    ss >> ref >> alt;
    p->PosVec.push_back(std::make_pair(chr, pos));
    p->ChooseBed[chr][pos] = std::make_pair(ref, alt);
  }
  return 0;
}
int read_ud(fq_popcon *p, const std::string &path) {   // ReadMatrixUD
  std::ifstream fin(path);
  if (!fin.is_open()) return p->fail(FQ_EIO, "Open file:" + path + "\t failed");
  std::string line;
  std::vector<double> tmpUD(p->numPC, 0);
  while (std::getline(fin, line)) {
    std::stringstream ss(line);
    for (int index = 0; index != p->numPC; ++index) ss >> tmpUD[index];
    p->UD.push_back(tmpUD);
    p->NumMarker++;
  }
  return 0;
}
int read_mean(fq_popcon *p, const std::string &path) {   // ReadMean
  std::ifstream fin(path);
  if (!fin.is_open()) return p->fail(FQ_EIO, "Open file:" + path + "\t failed");
  std::string line, snpName;
  double mu(0);
  while (std::getline(fin, line)) {
    std::stringstream ss(line);
    ss >> snpName;
    ss >> mu;
    p->means.push_back(mu);
  }
  return 0;
}
int read_af(fq_popcon *p, const std::string &path) {   // ReadAF
  std::ifstream fin(path);
  if (!fin.is_open()) return p->fail(FQ_EIO, "Open file:" + path + "\t failed");
  std::string line, chr;
  uint32_t pos(0);
  double AF(0);
  char ref(0), alt(0);
  while (std::getline(fin, line)) {
    std::stringstream ss(line);
    ss >> chr;
    ss >> pos >> pos;
    ss >> ref >> alt;
    ss >> AF;
    p->knownAF[chr][pos] = AF;
  }
  return 0;
}

void drop_packed(fq_popcon *p) {
  if (p->pd) { if (p->dev && !fqdev::bind(p->dev)) fqdev::pc_free(p->pd); p->pd = nullptr; }
  p->packed = false;
  p->cache.clear();
}
void clear_pileup(fq_popcon *p) {
  drop_packed(p);
  p->posIndex.clear();
  p->piles.clear();
  p->numBases = 0;
  p->effectiveNumSite = 0;
  p->avgDepth = 0;
  p->sdDepth = 0;
  p->have_pileup = p->sanity_done = p->sanity_failed = p->ran = false;
}

const Pile *pile_of(fq_popcon *p, uint32_t i) {
  auto c = p->posIndex.find(p->PosVec[i].first);
  if (c == p->posIndex.end()) return nullptr;
  auto q = c->second.find(p->PosVec[i].second);
  if (q == c->second.end()) return nullptr;
  return &p->piles[q->second];
}

// IsSanityCheckOK (ContaminationEstimator.cpp:493-536)
bool sanity_check(fq_popcon *p) {
  int tmpDepth(0);
  fprintf(stderr, "NOTICE - Number of marker in Reference Matrix:%d\n", (int)p->NumMarker);
  fprintf(stderr, "NOTICE - Number of marker shared with input file:%d\n", p->effectiveNumSite);
  for (size_t i = 0; i < p->NumMarker; ++i) {
    const Pile *pl = pile_of(p, (uint32_t)i);
    if (!pl) continue;
    tmpDepth = (int)pl->base.size();
    p->sdDepth += tmpDepth * tmpDepth;
  }
  p->sdDepth = sqrt(p->sdDepth / p->effectiveNumSite - p->avgDepth * p->avgDepth);
  p->effectiveNumSite = 0;
  for (size_t i = 0; i < p->NumMarker; ++i) {
    const Pile *pl = pile_of(p, (uint32_t)i);
    if (!pl) continue;
    tmpDepth = (int)pl->base.size();
    if (tmpDepth == 0 || tmpDepth < (p->avgDepth - 3 * p->sdDepth) || tmpDepth > (p->avgDepth + 3 * p->sdDepth)) continue;
    p->effectiveNumSite++;
  }
  fprintf(stderr, "NOTICE - Mean Depth:%f\n", p->avgDepth);
  fprintf(stderr, "NOTICE - SD Depth:%f\n", p->sdDepth);
  fprintf(stderr, "NOTICE - %d SNP markers remained after sanity check.\n", p->effectiveNumSite);
  return p->effectiveNumSite > 1000 and p->effectiveNumSite > (p->NumMarker * 0.1);
}

// the packed pileup of fq_popcon.h, in marker order; the device copy is made by k_pc_prepare from the characters themselves
int pack(fq_popcon *p) {
  if (p->packed) return 0;
  if (!p->have_pileup) return p->fail(FQ_EINVAL, "no pileup set");
  if (p->sanity_failed) return p->fail(FQ_ELIMIT, "Insufficient Available markers, check input bam depth distribution in output pileup file after specifying --OutputPileup");
  if (!p->o.disable_sanity_check && !p->sanity_done) {   // runVB2: IsSanityCheckOK stands before the first likelihood (it makes sdDepth)
    p->sanity_done = true;
    if (!sanity_check(p)) {
      p->sanity_failed = true;
      return p->fail(FQ_ELIMIT, "Insufficient Available markers, check input bam depth distribution in output pileup file after specifying --OutputPileup");
    }
    fprintf(stderr, "NOTICE - Passing Marker Sanity Check...\n");
  }
  const uint32_t M = p->NumMarker;
  const bool sanity = !p->o.disable_sanity_check;
  p->depth.assign(M, 0);
  p->off.assign((size_t)M + 1, 0);
  p->skip.assign(M, 0);
  p->alt.assign(M, 0);
  p->af_flat.assign(M, 0.);
  memset(p->slot_of_q, 0, sizeof p->slot_of_q);
  bool seen[256] = {};
  p->n_q = 0;
  std::vector<const Pile *> pl(M);
  uint64_t bytes = 0, n_chars = 0;
  p->markers_used = 0;
  for (uint32_t i = 0; i < M; ++i) {
    pl[i] = pile_of(p, i);
    const uint32_t d = pl[i] ? (uint32_t)pl[i]->base.size() : 0;
    p->depth[i] = d;
    p->off[i] = bytes;
    bytes += (d + (FQ_PC_PAD - 1)) & ~(uint64_t)(FQ_PC_PAD - 1);
    n_chars += d;
    p->skip[i] = fq_pc_skip(d, sanity, p->avgDepth, p->sdDepth) ? 1 : 0;
    p->markers_used += !p->skip[i];
    p->alt[i] = p->ChooseBed[p->PosVec[i].first][p->PosVec[i].second].second;
    if (p->isAFknown) p->af_flat[i] = p->knownAF[p->PosVec[i].first][(uint32_t)p->PosVec[i].second];
    for (uint32_t j = 0; j < d; ++j) {
      const uint8_t q = (uint8_t)pl[i]->qual[j];
      if (!seen[q]) {
        if (p->n_q == FQ_PC_MAXQ) return p->fail(FQ_ELIMIT, "the pileup holds more than 85 distinct quality characters");
        seen[q] = true;
        p->slot_of_q[q] = (uint8_t)p->n_q;
        p->q_of_slot[p->n_q++] = (int8_t)q;
      }
    }
  }
  p->off[M] = bytes;
  if (p->n_q == 0) { p->q_of_slot[0] = 33; p->n_q = 1; }
  p->code.assign(bytes + FQ_PC_PAD, 0);
  std::vector<char> base_flat(n_chars ? n_chars : 1), qual_flat(n_chars ? n_chars : 1);
  uint64_t r = 0;
  for (uint32_t i = 0; i < M; ++i)
    for (uint32_t j = 0; j < p->depth[i]; ++j, ++r) {
      base_flat[r] = pl[i]->base[j];
      qual_flat[r] = pl[i]->qual[j];
      p->code[p->off[i] + j] = (uint8_t)(p->slot_of_q[(uint8_t)pl[i]->qual[j]] * 3 + fq_pc_class(pl[i]->base[j], p->alt[i]));
    }
  p->ud_flat.assign((size_t)M * (p->numPC ? p->numPC : 1), 0.);
  for (uint32_t i = 0; i < M; ++i) for (int k = 0; k < p->numPC; ++k) p->ud_flat[(size_t)i * p->numPC + k] = p->UD[i][k];
  FqPcPile &P = p->hp;
  P.n_marker = (int32_t)M; P.n_pc = p->numPC; P.n_q = p->n_q; P.known_af = p->isAFknown;
  P.depth = p->depth.data(); P.off = p->off.data(); P.code = p->code.data(); P.skip = p->skip.data(); P.q_of_slot = p->q_of_slot;
  P.ud = p->ud_flat.data(); P.mean = p->means.data(); P.af = p->af_flat.data();
  if (!p->o.host_eval) {
    if (!p->dev) {
      p->dev = fqdev::state_create(p->o.device);
      if (!p->dev) return p->fail(FQ_ENODEV, std::string("pop+con: no device for the likelihood kernels (") + fqdev::last_error() + "); --host_eval runs the host loop");
    }
    if (fqdev::bind(p->dev)) return p->fail(FQ_ENODEV, fqdev::last_error());
    fqdev::FqPcPrepHost h{};
    h.n_marker = (int32_t)M; h.n_pc = p->numPC; h.n_q = p->n_q; h.known_af = p->isAFknown; h.sanity = sanity; h.avg = p->avgDepth; h.sd = p->sdDepth;
    h.depth = p->depth.data(); h.base = base_flat.data(); h.qual = qual_flat.data(); h.alt = p->alt.data(); h.n_chars = n_chars;
    h.slot_of_q = p->slot_of_q; h.q_of_slot = p->q_of_slot; h.ud = p->ud_flat.data(); h.mean = p->means.data(); h.af = p->af_flat.data();
    p->pd_points = kBatch;
    p->pd = fqdev::pc_prepare(h, p->pd_points);
    if (!p->pd) return p->fail(FQ_ENODEV, std::string("pop+con: ") + fqdev::last_error());
  }
  p->packed = true;
  return 0;
}

// ComputeMixLLKs on the host: per-marker values (threads over marker ranges), then the sum, serial in marker order
void host_marker_values(fq_popcon *p, const double *pt, std::vector<double> &val) {
  const FqPcPile &P = p->hp;
  std::vector<double> table((size_t)P.n_q * 27);
  for (int t = 0; t < P.n_q * 27; ++t) table[t] = fq_pc_table_entry(P, pt[2 * FQ_PC_MAXPC], t);
  val.assign(P.n_marker, 0.);
  int nt = p->o.host_threads > 0 ? p->o.host_threads : std::min(16, fq_host_cpus());
  if (P.off[P.n_marker] < (1u << 16)) nt = 1;
  nt = std::max(1, std::min(nt, 64));
  auto work = [&](int a, int b) { for (int i = a; i < b; ++i) val[i] = fq_pc_marker_host(P, table.data(), pt, i); };
  if (nt == 1) { work(0, P.n_marker); return; }
  std::vector<std::thread> th;
  const int step = (P.n_marker + nt - 1) / nt;
  for (int a = 0; a < P.n_marker; a += step) th.emplace_back(work, a, std::min(P.n_marker, a + step));
  for (auto &t : th) t.join();
}
double host_llk(fq_popcon *p, const double *pt) {
  std::vector<double> val;
  host_marker_values(p, pt, val);
  double sumLLK(0);
  for (double v : val) sumLLK += v;
  return sumLLK;
}

int eval_points(fq_popcon *p, const double *pts, int n, double *out) {   // pts: FQ_PC_POINT doubles each
  p->n_eval += n;
  if (p->o.host_eval) {
    for (int i = 0; i < n; ++i) out[i] = host_llk(p, pts + (size_t)i * FQ_PC_POINT);
    return 0;
  }
  if (fqdev::bind(p->dev)) return p->fail(FQ_ENODEV, fqdev::last_error());
  for (int a = 0; a < n; a += p->pd_points) {
    const int m = std::min(p->pd_points, n - a);
    if (fqdev::pc_llk(p->pd, pts + (size_t)a * FQ_PC_POINT, m, out + a)) return p->fail(FQ_ENODEV, std::string("pop+con: ") + fqdev::last_error());
  }
  return 0;
}

struct EvalError { int rc; };
void make_point(const fq_popcon *p, const std::vector<double> &pc1, const std::vector<double> &pc2, double alpha, std::vector<double> &pt) {
  pt.assign(FQ_PC_POINT, 0.);
  for (int k = 0; k < p->numPC; ++k) { pt[k] = pc1[k]; pt[FQ_PC_MAXPC + k] = pc2[k]; }
  pt[2 * FQ_PC_MAXPC] = alpha;
}
// ComputeMixLLKs(pc1, pc2, alpha): from the prefetched values when the point is among them
double mix(fq_popcon *p, const std::vector<double> &pc1, const std::vector<double> &pc2, double alpha) {
  std::vector<double> pt;
  make_point(p, pc1, pc2, alpha, pt);
  for (size_t i = 0; i < p->cache.size(); ++i)
    if (!memcmp(p->cache[i].first.data(), pt.data(), FQ_PC_POINT * 8)) {
      const double v = p->cache[i].second;
      p->cache.erase(p->cache.begin() + i);
      return v;
    }
  double v = 0;
  if (int rc = eval_points(p, pt.data(), 1, &v)) throw EvalError{rc};
  return v;
}
void prefetch_points(fq_popcon *p, const std::vector<std::vector<double>> &pts) {
  p->cache.clear();
  if (pts.size() < 2) return;
  std::vector<double> flat, vals(pts.size());
  for (auto &q : pts) flat.insert(flat.end(), q.begin(), q.end());
  if (int rc = eval_points(p, flat.data(), (int)pts.size(), vals.data())) throw EvalError{rc};
  for (size_t i = 0; i < pts.size(); ++i) p->cache.emplace_back(pts[i], vals[i]);
}

double inv_logit(double x) { double e = exp(x); return e / (1. + e); }
double logit(double x) { return log(x / (1. - x)); }

// what FullLLKFunc::Evaluate hands to ComputeMixLLKs for the simplex vector v (.h:306-400)
void model_args(const fq_popcon *p, const std::vector<double> &v, std::vector<double> &pc1, std::vector<double> &pc2, double &a) {
  const int n = p->numPC;
  if (!p->isHeter) {
    if (p->isPCFixed) { pc1 = p->fixPC; pc2 = p->fixPC2; a = inv_logit(v[0]); }
    else if (p->isAlphaFixed) { pc1.assign(v.begin(), v.begin() + n); pc2 = pc1; a = p->fixAlpha; }
    else { pc1.assign(v.begin(), v.begin() + n); pc2 = pc1; a = inv_logit(v[n]); }
  } else {
    if (p->isPCFixed) { pc1.assign(v.begin(), v.begin() + n); pc2 = p->fixPC2; a = inv_logit(v[n]); }
    else if (p->isAlphaFixed) { pc1.assign(v.begin(), v.begin() + n); pc2.assign(v.begin() + n, v.begin() + 2 * n); a = p->fixAlpha; }
    else { pc1.assign(v.begin(), v.begin() + n); pc2.assign(v.begin() + n, v.begin() + 2 * n); a = inv_logit(v[2 * n]); }
  }
}
// FullLLKFunc::Evaluate: the value, and "keep the best point seen"
double evaluate(fq_popcon *p, const std::vector<double> &v) {
  std::vector<double> pc1, pc2;
  double a = 0;
  model_args(p, v, pc1, pc2, a);
  const double smLLK = 0 - mix(p, pc1, pc2, a);
  if (smLLK < p->llk1) {
    p->llk1 = smLLK;
    if (!p->isHeter) {
      if (p->isPCFixed) p->globalAlpha = a;
      else if (p->isAlphaFixed) { p->globalPC = pc1; p->globalPC2 = pc1; }
      else { p->globalPC = pc1; p->globalPC2 = pc1; p->globalAlpha = a; }
    } else {
      if (p->isPCFixed) { p->globalPC = pc1; p->globalAlpha = a; }
      else if (p->isAlphaFixed) { p->globalPC = pc1; p->globalPC2 = pc2; }
      else { p->globalPC = pc1; p->globalPC2 = pc2; p->globalAlpha = a; }
    }
  }
  return smLLK;
}

// the Optimize* members (ContaminationEstimator.cpp:142-282): dimension and starting point by case, then the results back into PC / alpha
enum { OPT_HOMO, OPT_HOMO_FIXED_PC, OPT_HOMO_FIXED_ALPHA, OPT_HETER, OPT_HETER_FIXED_ALPHA };
void optimize(fq_popcon *p, Amoeba &mz, int which, bool *llk1_due) {   // *llk1_due: Initialize's likelihood travels with this stage's starting simplex
  const int n = p->numPC;
  std::vector<double> start;
  switch (which) {
    case OPT_HOMO: start = p->PC[0]; start.push_back(logit(p->alpha)); break;
    case OPT_HOMO_FIXED_PC: start.assign(1, logit(p->alpha)); break;
    case OPT_HOMO_FIXED_ALPHA: start = p->PC[0]; break;
    case OPT_HETER: start = p->PC[0]; start.insert(start.end(), p->PC[1].begin(), p->PC[1].end()); start.push_back(logit(p->alpha)); break;
    default: start = p->PC[0]; start.insert(start.end(), p->PC[1].begin(), p->PC[1].end()); break;
  }
  mz.f = [p](const std::vector<double> &v) { return evaluate(p, v); };
  mz.prefetch = [p, llk1_due](const std::vector<std::vector<double>> &vs) {
    std::vector<std::vector<double>> pts;
    const bool first = *llk1_due;
    if (first) { pts.emplace_back(); make_point(p, p->fixPC, p->fixPC2, p->fixAlpha, pts.back()); }
    for (auto &v : vs) {
      std::vector<double> pc1, pc2, pt;
      double a = 0;
      model_args(p, v, pc1, pc2, a);
      make_point(p, pc1, pc2, a, pt);
      pts.push_back(pt);
    }
    prefetch_points(p, pts);
    if (first) { *llk1_due = false; p->llk1 = (0 - mix(p, p->fixPC, p->fixPC2, p->fixAlpha)); }   // (before the first vertex is looked at, as Initialize has it)
  };
  mz.reset((int)start.size());
  mz.point = start;
  bool failed = false;
  mz.minimize(p->o.epsilon, &failed);
  switch (which) {
    case OPT_HOMO: p->alpha = inv_logit(mz.point[n]); for (int i = 0; i < n; ++i) p->PC[0][i] = mz.point[i]; break;
    case OPT_HOMO_FIXED_PC: p->alpha = inv_logit(mz.point[0]); break;
    case OPT_HOMO_FIXED_ALPHA: for (int i = 0; i < n; ++i) p->PC[0][i] = mz.point[i]; break;
    case OPT_HETER: p->alpha = inv_logit(mz.point[2 * n]);   // fall through
    default: for (int i = 0; i < n; ++i) { p->PC[0][i] = mz.point[i]; p->PC[1][i] = mz.point[n + i]; } break;
  }
}

// OptimizeLLK (ContaminationEstimator.cpp:29-76) with FullLLKFunc::Initialize and CalculateLLK0
void optimize_llk(fq_popcon *p) {
  Amoeba mz;
  p->n_eval = 0;
  // Initialize
  p->globalPC = p->fixPC = p->globalPC2 = p->fixPC2 = p->PC[1];
  p->globalAlpha = p->fixAlpha = p->alpha;
  bool llk1_due = true;   // llk1 = -ComputeMixLLKs(fixPC, fixPC2, fixAlpha): one launch with the first stage's starting simplex
  for (int k = 0; k < p->numPC; ++k) p->PC[0][k] = 0.01;
  for (int k = 0; k < p->numPC; ++k) p->PC[1][k] = 0.01;
  p->alpha = 0.03;
  if (!p->isHeter) {
    if (p->isPCFixed) optimize(p, mz, OPT_HOMO_FIXED_PC, &llk1_due);
    else if (p->isAlphaFixed) optimize(p, mz, OPT_HOMO_FIXED_ALPHA, &llk1_due);
    else optimize(p, mz, OPT_HOMO, &llk1_due);
  } else {
    if (p->isPCFixed) optimize(p, mz, OPT_HOMO, &llk1_due);   // OptimizeHeterFixedPC is OptimizeHomo, evaluated under isHeter
    else {
      const bool fa = p->isAlphaFixed;
      p->isHeter = false;
      optimize(p, mz, fa ? OPT_HOMO_FIXED_ALPHA : OPT_HOMO, &llk1_due);
      p->PC[1] = p->PC[0];
      p->globalPC2 = p->globalPC;
      p->isHeter = true;
      optimize(p, mz, fa ? OPT_HETER_FIXED_ALPHA : OPT_HETER, &llk1_due);
    }
    if (p->globalAlpha >= 0.5) {
      std::swap(p->globalPC[0], p->globalPC2[0]);
      std::swap(p->globalPC[1], p->globalPC2[1]);   // (components 0 and 1 only, as the reference; num_pc 1 is refused at create)
    }
  }
  p->llk0 = (0 - mix(p, p->globalPC, p->globalPC, 0));
}

}  // namespace

extern "C" {

void fq_popcon_default_opts(fq_popcon_opts_t *o) {
  memset(o, 0, sizeof *o);
  o->num_pc = 4;
  o->epsilon = 1e-8;
  o->fix_alpha_value = -1.;
}

int fq_popcon_create(const char *svd_prefix, const char *ud, const char *mu, const char *bed, const fq_popcon_opts_t *o, fq_popcon_t **out) {
  g_create_err.clear();
  if (!out) return FQ_EINVAL;
  *out = nullptr;
  fq_popcon_opts_t d;
  fq_popcon_default_opts(&d);
  if (o) d = *o;
  std::string udp, mup, bedp;
  if (svd_prefix) { udp = std::string(svd_prefix) + ".UD"; mup = std::string(svd_prefix) + ".mu"; bedp = std::string(svd_prefix) + ".bed"; }
  else if (ud && mu && bed) { udp = ud; mup = mu; bedp = bed; }
  else { g_create_err = "pop+con: an SVD prefix, or the .UD, .mu and .bed paths, are required"; return FQ_EINVAL; }
  if (d.num_pc < 1 || d.num_pc > FQ_PC_MAXPC) { g_create_err = "pop+con: num_pc must be 1..8"; return FQ_EINVAL; }
  const bool heter = !d.within_ancestry && !d.known_af;
  if (heter && d.num_pc < 2) {
    g_create_err = "pop+con: --NumPC 1 needs --WithinAncestry (the between-ancestry model exchanges components 1 and 2 of the two samples when alpha >= 0.5)";
    return FQ_EINVAL;
  }
  fq_popcon *p = new fq_popcon;
  p->o = d;
  p->numPC = d.num_pc;
  p->PC[0].assign(p->numPC, 0.);
  p->PC[1].assign(p->numPC, 0.);
  p->isHeter = !d.within_ancestry;
  if (d.fix_pc) { for (int i = 0; i < p->numPC; ++i) p->PC[1][i] = d.fix_pc_values[i]; p->isPCFixed = true; }
  else if (d.fix_alpha) { p->alpha = d.fix_alpha_value; p->isAlphaFixed = true; }
  int rc = read_bed(p, bedp);
  if (!rc && d.known_af) {
    p->known_af_path = d.known_af;
    p->o.known_af = p->known_af_path.c_str();
    p->isAFknown = true;
    p->isPCFixed = true;
    p->isHeter = false;
    rc = read_af(p, p->known_af_path);
  }
  if (!rc) rc = read_ud(p, udp);
  if (!rc) rc = read_mean(p, mup);
  if (!rc && p->NumMarker == 0) rc = p->fail(FQ_EIO, "pop+con: " + udp + " holds no marker");
  if (!rc && (p->PosVec.size() < p->NumMarker || p->means.size() < p->NumMarker))
    rc = p->fail(FQ_EIO, "pop+con: the .bed or the .mu file has fewer lines than the .UD file");
  if (rc) { g_create_err = p->err; delete p; return rc; }
  for (uint32_t i = 0; i < p->NumMarker; ++i) p->row_of[p->PosVec[i].first].emplace(p->PosVec[i].second, (int32_t)i);   // (the first row of a site stays)
  *out = p;
  return 0;
}

int fq_popcon_set_pileup_file(fq_popcon_t *p, const char *path) {   // SimplePileupViewer::ReadPileup
  if (!p || !path) return FQ_EINVAL;
  clear_pileup(p);
  int globalIndex = 0;
  std::string pChr;
  int pPos = 0;
  std::string refAllele;
  int depth = 0;
  std::string seq, qual;
  std::ifstream fin(path);
  if (!fin.is_open()) return p->fail(FQ_EIO, std::string("open file ") + path + " failed!");
  std::string pileupLine;
  while (getline(fin, pileupLine)) {
    std::stringstream ss(pileupLine);
    ss >> pChr >> pPos >> refAllele >> depth >> seq >> qual;
    if (seq.find_first_of(".,") != std::string::npos) {
      if (refAllele == ".") { clear_pileup(p); return p->fail(FQ_EINVAL, "Pileup format error: cannot find ref allele, exit!"); }
    }
    auto bc = p->ChooseBed.find(pChr);
    if (bc == p->ChooseBed.end()) continue;
    else if (bc->second.find(pPos) == bc->second.end()) continue;
    int tmpIndex(0);
    bool existed(false);
    auto &byPos = p->posIndex[pChr];
    auto it = byPos.find(pPos);
    if (it != byPos.end()) { tmpIndex = it->second; existed = true; }
    else { byPos[pPos] = globalIndex; tmpIndex = globalIndex; globalIndex++; p->piles.emplace_back(); }
    if (existed) fprintf(stderr, "[WARNING] The pileup file has duplicated lines! Merged here\n");
    Pile &pl = p->piles[tmpIndex];
    pl.base.insert(pl.base.end(), seq.begin(), seq.end());
    pl.qual.insert(pl.qual.end(), qual.begin(), qual.end());
    p->numBases += depth;
    depth = 0;
    seq = "";
    qual = "";
    p->effectiveNumSite++;
  }
  p->avgDepth = (double)p->numBases / p->effectiveNumSite;
  for (auto &pl : p->piles)
    if (pl.base.size() != pl.qual.size()) { clear_pileup(p); return p->fail(FQ_EINVAL, "pop+con: a pileup line's bases and qualities differ in length"); }
  p->have_pileup = true;
  p->isPileupInput = true;
  return 0;
}

int fq_popcon_set_pileup_arrays(fq_popcon_t *p, const int32_t *marker, const char *base, const char *qual, int64_t n) {
  if (!p || n < 0 || (n && (!marker || !base || !qual))) return FQ_EINVAL;
  clear_pileup(p);
  for (int64_t i = 0; i < n; ++i) {
    if (marker[i] < 0 || (uint32_t)marker[i] >= p->NumMarker) { clear_pileup(p); return p->fail(FQ_EINVAL, "pop+con: marker index out of range"); }
    const auto &pv = p->PosVec[marker[i]];
    auto &byPos = p->posIndex[pv.first];
    auto it = byPos.find(pv.second);
    int idx;
    if (it != byPos.end()) idx = it->second;
    else { idx = (int)p->piles.size(); byPos[pv.second] = idx; p->piles.emplace_back(); p->effectiveNumSite++; }
    p->piles[idx].base.push_back(base[i]);
    p->piles[idx].qual.push_back(qual[i]);
  }
  if (p->effectiveNumSite == 0) { clear_pileup(p); return p->fail(FQ_EINVAL, "pop+con: the pileup holds no base on any marker"); }
  p->numBases = n;
  p->avgDepth = (double)p->numBases / p->effectiveNumSite;
  p->have_pileup = true;
  p->isPileupInput = true;
  return 0;
}

int32_t fq_popcon_marker_index(const fq_popcon_t *p, const char *chrom, int32_t pos) {
  if (!p || !chrom) return -1;
  auto c = p->row_of.find(chrom);
  if (c == p->row_of.end()) return -1;
  auto r = c->second.find(pos);
  return r == c->second.end() ? -1 : r->second;
}
int fq_popcon_marker_alleles(const fq_popcon_t *p, int32_t marker, char *ref, char *alt) {
  if (!p || marker < 0 || (uint32_t)marker >= p->NumMarker) return FQ_EINVAL;
  const auto &pv = p->PosVec[marker];
  const auto &ra = p->ChooseBed.at(pv.first).at(pv.second);
  if (ref) *ref = ra.first;
  if (alt) *alt = ra.second;
  return 0;
}

static int to_points(fq_popcon *p, const double *points, int n, std::vector<double> &flat) {
  flat.assign((size_t)n * FQ_PC_POINT, 0.);
  for (int i = 0; i < n; ++i) {
    const double *s = points + (size_t)i * (2 * p->numPC + 1);
    double *d = flat.data() + (size_t)i * FQ_PC_POINT;
    for (int k = 0; k < p->numPC; ++k) { d[k] = s[k]; d[FQ_PC_MAXPC + k] = s[p->numPC + k]; }
    d[2 * FQ_PC_MAXPC] = s[2 * p->numPC];
  }
  return 0;
}

int fq_popcon_llk(fq_popcon_t *p, const double *points, int32_t n_points, double *out) {
  if (!p || !points || !out || n_points < 1) return FQ_EINVAL;
  if (int rc = pack(p)) return rc;
  std::vector<double> flat;
  to_points(p, points, n_points, flat);
  return eval_points(p, flat.data(), n_points, out);
}

int fq_popcon_marker_llk(fq_popcon_t *p, const double *point, double *out) {
  if (!p || !point || !out) return FQ_EINVAL;
  if (int rc = pack(p)) return rc;
  std::vector<double> flat;
  to_points(p, point, 1, flat);
  if (p->o.host_eval) {
    std::vector<double> val;
    host_marker_values(p, flat.data(), val);
    memcpy(out, val.data(), val.size() * 8);
    return 0;
  }
  if (fqdev::bind(p->dev)) return p->fail(FQ_ENODEV, fqdev::last_error());
  if (fqdev::pc_marker_llk(p->pd, flat.data(), out)) return p->fail(FQ_ENODEV, std::string("pop+con: ") + fqdev::last_error());
  return 0;
}

int fq_popcon_run(fq_popcon_t *p) {
  if (!p) return FQ_EINVAL;
  if (!p->have_pileup) return p->fail(FQ_EINVAL, "no pileup set");
  if (p->ran) return p->fail(FQ_EINVAL, "pop+con: the estimate has run (set a pileup again for another)");
  if (int rc = pack(p)) return rc;
  try { optimize_llk(p); } catch (const EvalError &e) { return e.rc; }
  p->ran = true;
  return 0;
}

int fq_popcon_result(const fq_popcon_t *p, fq_popcon_result_t *out) {
  if (!p || !out) return FQ_EINVAL;
  memset(out, 0, sizeof *out);
  if (!p->ran) return FQ_EINVAL;
  out->alpha = p->globalAlpha;
  for (int k = 0; k < p->numPC; ++k) { out->pc1[k] = p->globalPC[k]; out->pc2[k] = p->globalPC2[k]; }
  out->llk1 = p->llk1; out->llk0 = p->llk0; out->n_eval = p->n_eval;
  out->n_marker = (int32_t)p->NumMarker; out->markers_used = p->markers_used; out->num_pc = p->numPC;
  out->avg_depth = p->avgDepth; out->sd_depth = p->sdDepth;
  return 0;
}

int fq_popcon_write(fq_popcon_t *p, const char *out_prefix) {
  if (!p || !out_prefix) return FQ_EINVAL;
  if (!p->ran) return p->fail(FQ_EINVAL, "pop+con: nothing to write before fq_popcon_run");
  const std::string pre(out_prefix);
  {
    std::ofstream fout(pre + ".Ancestry");
    if (!fout.is_open()) return p->fail(FQ_EIO, "Open file " + pre + ".Ancestry failed!");
    fout << "PC\tContaminatingSample\tIntendedSample" << std::endl;
    for (int i = 0; i < p->numPC; ++i) fout << i + 1 << "\t" << p->globalPC[i] << "\t" << p->globalPC2[i] << std::endl;
    fout.close();
    if (!fout) return p->fail(FQ_EIO, "Errors detected when writing to file " + pre + ".Ancestry !");
  }
  {
    std::ofstream fout(pre + ".Summary", std::ios::app);
    if (!fout.is_open()) return p->fail(FQ_EIO, "Open file " + pre + ".Summary failed!");
    fout << "Contamination Level : " << (p->globalAlpha < 0.5 ? p->globalAlpha : (1 - p->globalAlpha)) << std::endl;
    fout.close();
    if (!fout) return p->fail(FQ_EIO, "Errors detected when writing to file " + pre + ".Summary !");
  }
  {
    const char *headers = "#SEQ_ID\tRG\tCHIP_ID\t#SNPS\t#READS\tAVG_DP\tFREEMIX\tFREELK1\tFREELK0\tFREE_RH\tFREE_RA\tCHIPMIX\tCHIPLK1\tCHIPLK0\tCHIP_RH\tCHIP_RA\tDPREF\tRDPHET\tRDPALT";
    std::ofstream fout(pre + ".selfSM");
    if (!fout.is_open()) return p->fail(FQ_EIO, "Open file " + pre + ".selfSM failed!");
    fout << headers << std::endl;
    fout << "DefaultSampleName" << "\tNA\tNA\t" << p->NumMarker << "\t";
    if (p->isPileupInput) fout << "NA";
    else fout << p->numBases;
    fout << "\t" << p->avgDepth << "\t" << ((p->globalAlpha < 0.5) ? p->globalAlpha : (1.f - p->globalAlpha)) << "\t" << -p->llk1 << "\t" << -p->llk0 << "\t"
         << "NA\tNA\t" << "NA\tNA\tNA\tNA\tNA\t" << "NA\tNA\tNA" << std::endl;
    fout.close();
    if (!fout) return p->fail(FQ_EIO, "Errors detected when writing to file " + pre + ".selfSM !");
  }
  return 0;
}

const char *fq_popcon_last_error(const fq_popcon_t *p) { return p ? p->err.c_str() : g_create_err.c_str(); }

void fq_popcon_destroy(fq_popcon_t *p) {
  if (!p) return;
  drop_packed(p);
  if (p->dev) fqdev::state_destroy(p->dev);
  delete p;
}

}  // extern "C"
