// popcon_gen.cpp -- generator of tests/golden/_popcon: drives VerifyBamID2's ContaminationEstimator (compiled from the reference tree, see README.md)
// over a pileup and records what fastquick_amd's pop+con is held to.  Never part of the product, never run by a test.
//
//   popcon_gen SVD_PREFIX PILEUP OUT_PREFIX NUM_PC [within] [nosanity] [fixpc=a:b:..] [fixalpha=x] [knownaf=FILE]
//
// writes OUT_PREFIX.golden (likelihood at fixed points, the estimates at Epsilon 1e-8 and 1e-10, %.17g) and, from the 1e-8 run,
// OUT_PREFIX.selfSM / .Ancestry / .Summary as runVB2 writes them.
//
// SimplePileupViewer.cpp needs htslib and cannot be compiled here: its empty constructor / destructor are defined below and the viewer's public
// fields are filled by fill_viewer(), a small restatement of ReadPileup's rules (sites outside the .bed skipped, duplicate sites merged, numBases
// adds the depth column, effectiveNumSite counts lines, avgDepth = numBases / effectiveNumSite, ref "." with ./, bases ends the run).
#include "ContaminationEstimator.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

SimplePileupViewer::SimplePileupViewer() {}
SimplePileupViewer::~SimplePileupViewer() {}
// (referred to by ContaminationEstimator::ReadBam / ReadPileup, which this driver never calls)
SimplePileupViewer::SimplePileupViewer(std::vector<region_t> *, const char *, const char *, const char *, int) { abort(); }
SimplePileupViewer::SimplePileupViewer(const BED &, const std::string &) { abort(); }

struct Args {
  std::string svd, pileup, out, knownaf;
  int num_pc = 4;
  bool within = false, nosanity = false, has_fixpc = false, has_fixalpha = false;
  std::vector<double> fixpc;
  double fixalpha = -1;
};

static void fill_viewer(ContaminationEstimator &E, const std::string &path) {
  SimplePileupViewer &V = E.viewer;
  std::ifstream in(path);
  if (!in.is_open()) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
  std::string line, chr, ref, seq, qual;
  int pos = 0, depth = 0, next = 0;
  V.numBases = 0;
  while (std::getline(in, line)) {
    std::stringstream ss(line);
    ss >> chr >> pos >> ref >> depth >> seq >> qual;
    if (ref == "." && seq.find_first_of(".,") != std::string::npos) { fprintf(stderr, "ref allele missing\n"); exit(1); }
    if (!E.ChooseBed.count(chr) || !E.ChooseBed[chr].count(pos)) continue;
    int at;
    if (V.posIndex.count(chr) && V.posIndex[chr].count(pos)) {
      at = V.posIndex[chr][pos];
      fprintf(stderr, "duplicate site merged\n");
    } else {
      at = next++;
      V.posIndex[chr][pos] = at;
      V.baseInfo.emplace_back();
      V.qualInfo.emplace_back();
    }
    V.baseInfo[at].insert(V.baseInfo[at].end(), seq.begin(), seq.end());
    V.qualInfo[at].insert(V.qualInfo[at].end(), qual.begin(), qual.end());
    V.numBases += depth;
    V.effectiveNumSite++;
    depth = 0;
    seq.clear();
    qual.clear();
  }
  V.avgDepth = (double)V.numBases / V.effectiveNumSite;
  E.isPileupInput = true;
}

// the set-up of runVB2 between the constructor and OptimizeLLK
static ContaminationEstimator *make(const Args &a, double eps, bool *sane) {
  const std::string bed = a.svd + ".bed";
  ContaminationEstimator *E = new ContaminationEstimator(a.num_pc, bed.c_str(), 1, eps);
  E->verbose = false;
  E->seed = 12345;
  E->isHeter = !a.within;
  E->isSanityCheckDisabled = a.nosanity;
  if (a.has_fixpc) { for (int i = 0; i < a.num_pc; ++i) E->PC[1][i] = a.fixpc[i]; E->isPCFixed = true; }
  else if (a.has_fixalpha) { E->alpha = a.fixalpha; E->isAlphaFixed = true; }
  if (!a.knownaf.empty()) { E->isAFknown = true; E->isPCFixed = true; E->isHeter = false; E->ReadAF(a.knownaf); }
  E->ReadSVDMatrix(a.svd + ".UD", "", a.svd + ".mu");
  fill_viewer(*E, a.pileup);
  *sane = true;
  if (!a.nosanity) *sane = E->IsSanityCheckOK();
  return E;
}

static void put_vec(FILE *f, const char *key, const std::vector<double> &v) {
  fprintf(f, " %s", key);
  for (double x : v) fprintf(f, " %.17g", x);
}

int main(int argc, char **argv) {
  if (argc < 5) { fprintf(stderr, "usage: popcon_gen SVD_PREFIX PILEUP OUT_PREFIX NUM_PC [options]\n"); return 2; }
  Args a;
  a.svd = argv[1]; a.pileup = argv[2]; a.out = argv[3]; a.num_pc = atoi(argv[4]);
  for (int i = 5; i < argc; ++i) {
    const std::string s = argv[i];
    if (s == "within") a.within = true;
    else if (s == "nosanity") a.nosanity = true;
    else if (s.rfind("fixpc=", 0) == 0) {
      a.has_fixpc = true;
      std::stringstream ss(s.substr(6));
      std::string tok;
      while (std::getline(ss, tok, ':')) a.fixpc.push_back(atof(tok.c_str()));
    } else if (s.rfind("fixalpha=", 0) == 0) { a.has_fixalpha = true; a.fixalpha = atof(s.c_str() + 9); }
    else if (s.rfind("knownaf=", 0) == 0) a.knownaf = s.substr(8);
    else { fprintf(stderr, "unknown option %s\n", s.c_str()); return 2; }
  }
  FILE *g = fopen((a.out + ".golden").c_str(), "w");
  if (!g) return 2;
  bool sane = false;
  {
    ContaminationEstimator *E = make(a, 1e-8, &sane);
    fprintf(g, "num_marker %u\nmarkers_remained %d\nsane %d\navg_depth %.17g\nsd_depth %.17g\n", E->NumMarker, E->viewer.GetNumMarker(), sane ? 1 : 0, E->viewer.avgDepth, E->viewer.sdDepth);
    // the likelihood at eight fixed points: PC1, PC2, alpha
    const double alphas[8] = {0.5, 0.03, 0.001, 0.25, 0.9, 1e-9, 0.4999, 0.1};
    for (int t = 0; t < 8 && sane; ++t) {
      std::vector<double> p1(a.num_pc), p2(a.num_pc);
      for (int k = 0; k < a.num_pc; ++k) {
        p1[k] = t == 0 ? 0. : 0.01 * (k + 1) * (t - 3.5) + 0.002 * t;
        p2[k] = t < 2 ? p1[k] : -0.015 * (k + 1) * (t - 2.5) + 0.001 * k;
      }
      const double v = E->fn.ComputeMixLLKs(p1, p2, alphas[t]);
      fprintf(g, "point");
      put_vec(g, "pc1", p1);
      put_vec(g, "pc2", p2);
      fprintf(g, " alpha %.17g llk %.17g\n", alphas[t], v);
    }
    delete E;
  }
  const double eps[2] = {1e-8, 1e-10};
  for (int r = 0; r < 2 && sane; ++r) {
    ContaminationEstimator *E = make(a, eps[r], &sane);
    const std::string pre = r == 0 ? a.out : a.out + ".eps10";
    remove((pre + ".Summary").c_str());
    E->OptimizeLLK(pre);
    fprintf(g, "final eps %g alpha %.17g", eps[r], E->fn.globalAlpha);
    put_vec(g, "pc1", E->fn.globalPC);
    put_vec(g, "pc2", E->fn.globalPC2);
    fprintf(g, " llk1 %.17g llk0 %.17g\n", E->fn.llk1, E->fn.llk0);
    if (r == 0) {   // the row of runVB2's .selfSM
      std::ofstream o(a.out + ".selfSM");
      o << "#SEQ_ID\tRG\tCHIP_ID\t#SNPS\t#READS\tAVG_DP\tFREEMIX\tFREELK1\tFREELK0\tFREE_RH\tFREE_RA\tCHIPMIX\tCHIPLK1\tCHIPLK0\tCHIP_RH\tCHIP_RA\tDPREF\tRDPHET\tRDPALT" << std::endl;
      o << E->viewer.SEQ_SM << "\tNA\tNA\t" << E->NumMarker << "\t" << "NA" << "\t" << E->viewer.avgDepth << "\t"
        << ((E->fn.globalAlpha < 0.5) ? E->fn.globalAlpha : (1.f - E->fn.globalAlpha)) << "\t" << -E->fn.llk1 << "\t" << -E->fn.llk0
        << "\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA" << std::endl;
    } else {
      remove((pre + ".Summary").c_str());
      remove((pre + ".Ancestry").c_str());
    }
    delete E;
  }
  fclose(g);
  return sane ? 0 : 1;
}
