// fq_cli.cpp -- `FASTQuick_amd align`: the reference's `FASTQuick align --sam_out` command line on top of the C ABI.
//
// Mirrors runAlign (src/FASTQuick.cpp:159-488): same flag names and meanings for the flags the hot path reads, the
// index prefix convention (<index_prefix>.FASTQuick.fa.*), SAM text on stdout in the --sam_out dialect, the summary
// notices on stderr.  The FASTQ tokenizer follows kseq_read3_fpc (libbwa/kseq.h:327-370): name up to the first white
// space, bases = printable characters up to the '+' line, quality = exactly as many characters as bases.
// Without --sam_out the records go to <out_prefix>.bam in genome coordinates (fq_bam_*: SetSamRecord / SetSamFileHeader); the QC
// files of StatCollector (<out_prefix>.InsertSizeTable .Pileup .DepthDist ... .Summary) are written in both modes (fq_qc_*) when the
// index carries its .SelectedSite.vcf / .dbSNP.subset.vcf / .gc.  Flank lengths and the original reference (for @SQ and the genome
// size) come from <index_prefix>.FASTQuick.fa.param as `FASTQuick index` wrote it (src/FASTQuick.cpp:376-465).
#include <cmath>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <chrono>
#include <cstdio>
#include <map>
#include <functional>
#include <memory>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <fstream>
#include <vector>

#include "../../include/fastquick_amd.h"

// The estimator's entries are weak references here: the host-loop library of the CPU test tier (tests/emu) is built from the alignment sources alone, and
// this file links against it too; there `pop+con` and `align --popcon_svd` say that the build has no estimator.
#pragma weak fq_popcon_default_opts
#pragma weak fq_popcon_create
#pragma weak fq_popcon_set_pileup_file
#pragma weak fq_popcon_set_pileup_arrays
#pragma weak fq_popcon_marker_index
#pragma weak fq_popcon_marker_alleles
#pragma weak fq_popcon_run
#pragma weak fq_popcon_result
#pragma weak fq_popcon_write
#pragma weak fq_popcon_last_error
#pragma weak fq_popcon_destroy
#pragma weak fq_svd_default_opts
#pragma weak fq_svd_create
#pragma weak fq_svd_read_vcf
#pragma weak fq_svd_read_panel
#pragma weak fq_svd_read_stats
#pragma weak fq_svd_run
#pragma weak fq_svd_result
#pragma weak fq_svd_write
#pragma weak fq_svd_last_error
#pragma weak fq_svd_destroy

namespace {
// part / worker files of a multi-device run: removed when the run dies (a finished run appends and removes them itself)
std::mutex g_tmp_mu;
std::vector<std::string> g_tmp_files;
void tmp_file(const std::string &p) { std::lock_guard<std::mutex> lk(g_tmp_mu); g_tmp_files.push_back(p); }
// (_exit after flushing: other threads may be inside the HIP runtime -- the index is staged beside the first read -- and must not meet the
//  process's static destructors half-way)
[[noreturn]] void die(const std::string &m) {
  fprintf(stderr, "FATAL ERROR - \n%s\n", m.c_str());
  { std::lock_guard<std::mutex> lk(g_tmp_mu); for (const auto &p : g_tmp_files) remove(p.c_str()); }
  fflush(nullptr);
  _exit(EXIT_FAILURE);
}
// FASTQUICK_TRACE=1: wall-clock marks of the run's phases on stderr (milliseconds since the process began)
const std::chrono::steady_clock::time_point g_t0 = std::chrono::steady_clock::now();
const bool g_trace = [] { const char *e = getenv("FASTQUICK_TRACE"); return e && *e && *e != '0'; }();
// device objects being destroyed beside the run's next steps: release_later() starts, release_join() waits (before the index they refer to goes, and
// at the end).  (The list is never destroyed itself: a die() while a release runs must not meet a joinable thread in a static destructor.)
std::mutex g_releases_mu;
std::vector<std::thread> &releases() { static std::vector<std::thread> *v = new std::vector<std::thread>; return *v; }
template <class F> void release_later(F f) { std::lock_guard<std::mutex> lk(g_releases_mu); releases().emplace_back(std::move(f)); }
void release_join() {
  std::vector<std::thread> mine;
  { std::lock_guard<std::mutex> lk(g_releases_mu); mine.swap(releases()); }
  for (auto &t : mine) t.join();
}
void mark(const char *what) { if (g_trace) fprintf(stderr, "TRACE - %9.1f ms  %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - g_t0).count(), what); }
void notice(const char *fmt, long long a) { fprintf(stderr, "NOTICE - "); fprintf(stderr, fmt, a); fputc('\n', stderr); }

// One FASTQ file through the library's front end (fq_fastq_*: parallel inflate + tokeniser with kseq_read3_fpc's tokens)
struct FastqReader {
  fq_fastq_t *h = nullptr;
  std::string path;
  bool told_dropped = false;
  FastqReader(const std::string &p, int threads, int batch_pairs, int slot_mode, double frac) : path(p) {
    if (fq_fastq_open(p.c_str(), threads, &h)) die("Open " + p + " failed!");
    fq_fastq_configure(h, batch_pairs, slot_mode, 0);
    if (fq_fastq_set_sampling(h, frac)) die("--frac_samp must not be negative");
  }
  FastqReader(const std::string &p, fq_fastq_t *adopt) : h(adopt), path(p) {}      // a reader the device front end handed over (fq_frontend_handover)
  ~FastqReader() { if (h) fq_fastq_close(h); }
  FastqReader(const FastqReader &) = delete;
};
// length of a file's first read (0: none), to size the rows
size_t first_read_len(const std::string &path) {
  fq_fastq_t *h = nullptr;
  if (fq_fastq_open(path.c_str(), 1, &h)) return 0;
  fq_fastq_configure(h, 1, FQ_FASTQ_SLOTS_FRESH, 1 << 16);
  std::vector<uint8_t> seq(65536), qual(65536);
  std::vector<char> nm(512);
  int32_t len = 0;
  fq_fastq_rows_t rows = {65536, 512, seq.data(), qual.data(), &len, nm.data()};
  const int64_t n = fq_fastq_read(h, 1, &rows);
  fq_fastq_close(h);
  return n == 1 ? (size_t)len : 0;
}

struct Args {
  std::string fq1, fq2, out_prefix = "Empty", index_prefix = "Empty";
  bool sam_out = false;
  fq_opts_t o;
  int opte = -1;
  long long chunk_pairs = 16LL * 262144;
  int device = 0;
  std::string devices;   // --devices: several devices, the lines of --fq_list dealt over them
  int pack_threads = std::min(32, std::max(1, fq_host_cpus()));     // host threads of the FASTQ readers (half per file) and of the packer, from the CPUs the process may use; --t sets it
  bool clean_names = false;
  int bam_deflate = -1;          // --bam_deflate fixed|dynamic: how the device compresses the BAM file's members (FQ_DEFLATE_*; -1: not given, the writer's default or FASTQUICK_BAM_DEFLATE)
  bool sorted_bam = false;       // --sorted_bam: <out_prefix>.sorted.bam in coordinate order and its .bai instead of <out_prefix>.bam (fq_bam_create_sorted: what the pipeline's samtools sort / index steps made of O.bam)
  long long sort_mem = 4ll << 30; // --sort_mem: bytes of records the sorted writer keeps in host memory before its runs go to files
  std::string bam_file() const { return out_prefix + (sorted_bam ? ".sorted.bam" : ".bam"); }
  bool host_consumers = false;   // --host_consumers: SAM text and StatCollector's sums on the host's threads from the result arrays (round 5's way; the default runs them in kernels, fq_emit.h)
  bool host_reader = false;   // --host_reader: the FASTQ front end on the host's threads also for BGZF files (the default inflates and tokenises them on the device)
  bool strict = false;   // --strict_reference: stop where the output could differ from the reference's bytes (today: QUAL of reads of unequal lengths)
  bool collate = false;       // --collate: the mates of --bam_in are found by name across the file (fq_frontend_open_bam_collate: coordinate-sorted input)
  long long collate_mem = 4ll << 30;   // --collate_mem: bytes the records waiting for their mates may take in device memory
  bool collate_mem_given = false;
  std::string bam_in;         // --bam_in: one BAM file in place of the FASTQ files (fq_frontend_open_bam: its records are transcoded to FASTQ text on the device)
  std::vector<std::string> bam_rg;   // --bam_rg ID (repeatable): only the records of --bam_in whose RG:Z is one of these are read (fq_frontend_open_bam_select)
  bool bam_oq = false;        // --bam_oq: a record that has OQ:Z gives that as its quality line (the sequencer's qualities of a recalibrated file)
  int bam_l_seq = 0;          // ... the first kept record's length (fq_bam_probe): sizes the rows as a FASTQ file's first record does
  std::string fq_list, rg = "@RG\\tID:foo\\tSM:bar";   // runAlign's default --RG (src/FASTQuick.cpp:170)
  bool cal_dup = true;
  std::string popcon_svd;     // --popcon_svd P: after the QC files, the contamination and ancestry estimate (pop+con) on the marker pileups the QC consumer holds; P.UD / P.mu / P.bed
  bool popcon_within = false; // --popcon_within: pop+con's --WithinAncestry
  int popcon_numpc = 4;       // --popcon_numpc: pop+con's --NumPC
  double frac = 1.0;    // --frac_samp: gap_opt_t::frac (libbwa/bwtaln.c:47), the share of the records that is kept
  int read_len = 151;   // gap_opt_t::read_len (libbwa/bwtaln.c:48): the reference sizes its read buffers from it and has no flag for it
};

int usage() {
  fprintf(stderr, "Usage: FASTQuick_amd align --index_prefix P --fastq_1 R1.fq[.gz] [--fastq_2 R2.fq[.gz]] | --fq_list LIST | --bam_in X.bam [--collate [--collate_mem BYTES]] [--bam_rg ID]... [--bam_oq]  --out_prefix O [--sam_out | --sorted_bam [--sort_mem BYTES]] [--bam_deflate fixed|dynamic] [--RG STR] [--cal_dup]\n"
                  "                       [--q INT] [--n FLOAT|INT] [--kmer_thresh INT] [--o INT] [--e INT] [--i INT] [--d INT] [--l INT] [--k INT]\n"
                  "                       [--m INT] [--R INT] [--N] [--L] [--I] [--max_isize INT] [--max_occ INT] [--is_sw] [--n_multi INT] [--N_multi INT]\n"
                  "                       [--ap_prior FLOAT] [--force_isize] [--frac_samp FLOAT] [--t INT] [--chunk_pairs INT] [--batch_pairs INT] [--device INT | --devices LIST] [--read_len INT] [--clean_names] [--strict_reference] [--host_reader] [--host_consumers] [--popcon_svd P [--popcon_within] [--popcon_numpc INT]]\n"
                  "       FASTQuick_amd index --ref REDUCED.FASTQuick.fa [--rollhash]\n"
                  "       FASTQuick_amd pop+con --PileupFile F --SVDPrefix P | --UDPath U --MeanPath M --BedPath B  --Output O [--NumPC INT] [--WithinAncestry] [--FixPC a:b:..] [--FixAlpha FLOAT] [--KnownAF F]\n"
                  "                       [--DisableSanityCheck] [--Epsilon FLOAT] [--host_eval] [--device INT]\n"
                  "       FASTQuick_amd svd --RefVCF PANEL.vcf[.gz] | --RefVCFList LIST  [--Sites SITES.vcf] [--Output P] [--reader serial|device|host_loops] [--chunk_bytes INT] [--host_eval] [--device INT]\n");
  return 1;
}


using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

const int kNameStride = 304;   // the reference's name buffers hold 302 bytes (bwaseqio.c:233)
// Rows hold read_len bases, or the first records' if those are longer (fq2 empty: single-end) -- probed only in regular files (a pipe cannot
// be read twice: there a longer read is an error that asks for --read_len)
int row_stride(const Args &A, const std::string &fq1, const std::string &fq2) {
  auto regular = [](const std::string &p) { struct stat s; return stat(p.c_str(), &s) == 0 && S_ISREG(s.st_mode); };
  size_t l = 0;
  if (!A.bam_in.empty()) l = (size_t)A.bam_l_seq;
  else if (regular(fq1) && (fq2.empty() || regular(fq2))) l = std::max(first_read_len(fq1), fq2.empty() ? (size_t)0 : first_read_len(fq2));
  return (int)((std::max<size_t>(l, (size_t)std::max(A.read_len, 16)) + 15) & ~(size_t)15);
}

// grow-only storage that is not cleared on allocation: a chunk of the default size is 2.7 GB of rows, rows are cleared as
// records arrive, and value-initialising the rest cost seconds per run
template <class T> struct RawBuf {
  std::unique_ptr<T[]> p;
  size_t n = 0;
  void resize(size_t m) { if (m > n) { p.reset(new T[m]); n = m; } }     // (contents are not kept: callers fill what they use)
  size_t size() const { return n; }
  T *data() { return p.get(); }
  const T *data() const { return p.get(); }
  T &operator[](size_t i) { return p[i]; }
  const T &operator[](size_t i) const { return p[i]; }
};
// One end of one chunk: fixed-stride rows, filled by that file's reader thread.
struct EndChunk {
  uint8_t *seq = nullptr, *qual = nullptr;   // this end's rows in its chunk's buffers
  int32_t *len = nullptr;
  RawBuf<char> names;
  int n = 0;
  bool eof = false;
  std::string error;
};
// Reads up to `cap` records of one FASTQ file into `c` (rows of `stride` bytes; a read longer than that is an error: the
// reference, too, wants reads of one length, kseq.h:362-365).  The read-slot history of the reference (names without terminator,
// bases behind a short read: SURVEY Q7 / Q8) is modelled by the reader (fq_fastq_configure).
// (rows are cleared as records arrive: a chunk of the default size is 2.7 GB of rows, a small input touches a few of them)
void fill_end(FastqReader &r, EndChunk &c, long long cap, int stride) {
  c.n = 0; c.error.clear();
  fq_fastq_rows_t rows = {stride, kNameStride, c.seq, c.qual, c.len, c.names.data()};
  const int64_t n = fq_fastq_read(r.h, cap, &rows);
  if (n < 0) { c.error = fq_fastq_last_error(r.h); if (c.error.empty()) c.error = "reading " + r.path + " failed (" + std::to_string(n) + ")"; return; }
  c.n = (int)n;
  if (n < cap) c.eof = true;
  if (!r.told_dropped && fq_fastq_dropped_record(r.h)) {
    r.told_dropped = true;
    fprintf(stderr, "NOTICE - the last record (%s) has no line end after its quality string; like the reference's reader, it is not used\n", fq_fastq_dropped_record(r.h));
  }
}
// One chunk of a paired-end (two ends) or single-end (one) input in the layout fq_read_batch_t wants, [end][row][stride]: each file's reader
// fills its end in place, end 1 behind the `cap` rows of end 0; squeeze() moves it down behind the n rows of a short (last) chunk.
struct Chunk {
  int ends = 0, stride = 0;
  long long cap = 0;
  RawBuf<uint8_t> seq, qual;
  RawBuf<int32_t> len;
  EndChunk e[2];
  int n = 0;               // records per end (the shorter end's, if the files disagree)
  bool last = false;       // nothing follows this chunk
  long long index = -1;    // (the sharded run's bookkeeping: the chunk's number; -1 free, -2 being read)
  void init(int ends_, long long cap_, int stride_) {
    ends = ends_; cap = cap_; stride = stride_;
    seq.resize((size_t)ends * cap * stride); qual.resize((size_t)ends * cap * stride); len.resize((size_t)ends * cap);
    for (int k = 0; k < ends; ++k) {
      e[k].seq = seq.data() + (size_t)k * cap * stride; e[k].qual = qual.data() + (size_t)k * cap * stride; e[k].len = len.data() + (size_t)k * cap;
      e[k].names.resize((size_t)cap * kNameStride);
    }
  }
  void fill(FastqReader *const r[2]) {     // one thread per file (the reference, too, decodes the two files on two IO threads: BwtMapper.cpp:1873-1935)
    std::thread t0;
    if (ends == 2) t0 = std::thread(fill_end, std::ref(*r[0]), std::ref(e[0]), cap, stride);
    fill_end(*r[ends - 1], e[ends - 1], cap, stride);
    if (t0.joinable()) t0.join();
    const EndChunk &a = e[0], &b = e[ends - 1];
    n = std::min(a.n, b.n);
    last = n == 0 || a.eof || b.eof || a.n != b.n;
  }
  const std::string &error() const { return !e[0].error.empty() ? e[0].error : e[ends - 1].error; }   // the first reader's first
  void squeeze() {
    if (ends < 2 || (long long)n >= cap) return;
    memmove(seq.data() + (size_t)n * stride, e[1].seq, (size_t)n * stride);
    memmove(qual.data() + (size_t)n * stride, e[1].qual, (size_t)n * stride);
    memmove(len.data() + n, e[1].len, (size_t)n * sizeof(int32_t));
  }
  fq_read_batch_t batch() const { return {n, stride, seq.data(), qual.data(), len.data(), e[0].names.data(), kNameStride, ends == 2 ? e[1].names.data() : nullptr}; }
  const char *first_name(int sb, int end, int batch_pairs) const { return &e[end].names[(size_t)sb * batch_pairs * kNameStride]; }   // of reference batch sb
};

// Where a worker's records go.  One device: straight to stdout / the BAM file, as they are produced.  Several devices: every FASTQ pair
// of a list into part files of its own (SAM text; BAM records as bytes), which the main thread appends to the output in input order; every
// chunk of a sharded pair into memory, which the run's writer appends in chunk order.
struct Sink {
  FILE *sam_fp = nullptr;            // stdout, or the input's part file
  fq_bam_t *bam = nullptr;           // the file's writer (direct), or a formatter without a file
  FILE *bam_fp = nullptr;            // the input's part file of BAM records (null: direct)
  std::vector<char> *mem = nullptr;  // instead of either file: the records (SAM text, or BAM records as bytes) are appended here
  std::string what;
  void put(FILE *fp, const void *p, size_t n) {
    if (mem) mem->insert(mem->end(), (const char *)p, (const char *)p + n);
    else if (fwrite(p, 1, n, fp) != n) die("writing " + what + " failed");
  }
  void sam(const void *p, size_t n) { put(sam_fp, p, n); }
  void bam_add(fq_ctx_t *ctx) {
    if (!bam_fp && !mem) { if (fq_bam_add_last(bam, ctx)) die("writing " + what + " failed"); return; }
    const void *data = nullptr; int64_t len = 0;
    if (fq_bam_format_last(bam, ctx, &data, &len)) die("writing " + what + " failed");
    put(bam_fp, data, (size_t)len);
  }
  void records(const std::vector<char> &r) {   // what another sink gathered in memory, onto a direct one
    if (sam_fp) sam(r.data(), r.size());
    else if (fq_bam_write_records(bam, r.data(), (int64_t)r.size())) die("writing " + what + " failed");
  }
  void flush() { if (sam_fp) fflush(sam_fp); if (bam_fp) fflush(bam_fp); }
};
Sink direct_sink(const Args &A) {   // (.bam: set once the writer is there)
  Sink s;
  s.sam_fp = A.sam_out ? stdout : nullptr; s.what = A.sam_out ? "the SAM text" : A.bam_file();
  return s;
}
// The records of the context's last call, to the sink: SAM text formatted on the device or by the host, or BAM records.
void fetch_records(const Args &A, fq_ctx_t *cx, Sink &out) {
  if (!A.sam_out) out.bam_add(cx);
  else if (!A.host_consumers) {
    if (fq_sam_device_last(cx, [](void *user, const void *data, int64_t n) -> int { ((Sink *)user)->sam(data, (size_t)n); return 0; }, &out) < 0)
      die(std::string("fetching the SAM text failed: ") + fq_ctx_last_error(cx));
  } else {
    const int64_t sz = fq_sam_format_last(cx, nullptr, 0);
    std::vector<char> text((size_t)sz + 1);
    fq_sam_format_last(cx, text.data(), sz + 1);
    out.sam(text.data(), (size_t)sz);
  }
}
// A refusal ends the run behind the records of every call before it (the reference prints the batches before the one that aborts,
// src/BwtMapper.cpp:2030-2092): the caller has waited for whatever still produces records; the sink is flushed, then die().
[[noreturn]] void refuse_run(Sink &out, const std::string &m) { out.flush(); die(m); }
// The consumers of a context's records run in kernels inside its calls (fq_emit.h): the SAM text is formatted on the device, StatCollector's sums
// stay there, nothing on the host reads the result arrays any more (they stay in HBM); the host's consumers only move text and append.
void attach_device_consumers(fq_ctx_t *ctx, const Args &A, fq_bam_t *bam, fq_qc_t *qc) {
  if (A.host_consumers) return;
  if (fq_ctx_set_emit(ctx, (A.sam_out ? FQ_EMIT_SAM : 0) | FQ_EMIT_DEVICE_ONLY)) die("fq_ctx_set_emit failed");
  if (!A.sam_out && bam && fq_ctx_attach_bam(ctx, bam)) die("fq_ctx_attach_bam failed");
  if (qc && fq_ctx_attach_qc(ctx, qc)) die("fq_ctx_attach_qc failed");
}
// What a shard consumer gathered since its last export, as a segment for fq_qc_merge; the consumer starts its next segment.
void qc_export_segment(fq_qc_t *qc, std::vector<char> &seg) {
  const int64_t need = fq_qc_state_export(qc, nullptr, 0);
  if (need < 0) die(std::string("QC consumer: export failed: ") + fq_qc_last_error(qc));
  seg.resize((size_t)need);
  if (fq_qc_state_export(qc, seg.data(), need) != need || fq_qc_state_reset(qc)) die("QC consumer: export failed");
}
void write_sam_header(const fq_index_t *ix) {
  const int64_t n = fq_sam_header(ix, nullptr, 0);
  std::vector<char> h((size_t)n + 1);
  fq_sam_header(ix, h.data(), n + 1);
  fwrite(h.data(), 1, (size_t)n, stdout);
}
// src/BwtMapper.cpp:2087-2092: the first pair of a reference batch is compared when the running read count is a multiple of the batch
// size (every full batch; a short last batch normally is not checked), over read_len name bytes.  Mates whose names differ elsewhere
// pass, each printed under its own name (the reference's example input has such pairs).  first_name(sb, e): the first name of reference
// batch sb of the chunk, end e.  True: the run must abort with kOutOfOrder.
const char *const kOutOfOrder = "Abort, please make sure input pair of fastq files are in the same order!";
template <class F> bool order_check(const Args &A, long long &checked_reads, int n, F first_name) {
  for (int i = 0; i < n; i += A.o.batch_pairs) {
    checked_reads += 2LL * std::min<long long>(A.o.batch_pairs, n - i);
    if (checked_reads % A.o.batch_pairs == 0 && strncmp(first_name(i / A.o.batch_pairs, 0), first_name(i / A.o.batch_pairs, 1), (size_t)A.read_len) != 0) return true;
  }
  return false;
}
// the reference's closing lines of an input (counts of reads for a single-end input, of pairs doubled for a paired-end one)
void end_of_input_notices(bool se, long long num_read, long long filtered, long long unmapped) {
  if (!se) notice("%lld sequences are loaded.", num_read);
  notice("%lld sequences are filtered.", se ? filtered : filtered * 2);
  notice("%lld sequences are unmapped.", se ? unmapped : unmapped * 2);
}
// "0-3", "0,2,5", "0,0": the devices of --devices (a device named twice gets two workers)
std::vector<int> parse_devices(const std::string &v) {
  std::vector<int> d;
  auto ordinal = [&](const std::string &t) -> int {       // digits only: "a", "0-x", "1.5" are errors, not device 0
    char *e = nullptr;
    const long x = t.empty() ? -1 : strtol(t.c_str(), &e, 10);
    if (t.empty() || !e || *e || t.find_first_not_of("0123456789") != std::string::npos || x < 0 || x > 63) die("--devices: bad device ordinal '" + t + "' in " + v);
    return (int)x;
  };
  size_t at = 0;
  while (at < v.size()) {
    size_t end = v.find(',', at);
    if (end == std::string::npos) end = v.size();
    const std::string tok = v.substr(at, end - at);
    const size_t dash = tok.find('-');
    if (tok.empty()) die("--devices: empty entry in " + v);
    if (dash == std::string::npos) d.push_back(ordinal(tok));
    else { const int a = ordinal(tok.substr(0, dash)), b = ordinal(tok.substr(dash + 1)); if (b < a) die("--devices: bad range " + tok); for (int x = a; x <= b; ++x) d.push_back(x); }
    at = end + 1;
  }
  if (d.empty() || (!v.empty() && v.back() == ',')) die("--devices: empty entry in " + v);
  return d;
}
void append_file(const std::string &path, FILE *to, fq_bam_t *bam) {   // a part file onto the output (SAM text to `to`, BAM records to `bam`), then gone
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) die("cannot reopen " + path);
  std::vector<char> buf((size_t)8 << 20);
  size_t n, held = 0;      // (BAM records go on whole: a sorted writer takes every piece as a run of records; what a read cut off waits for the next)
  while ((n = fread(buf.data() + held, 1, buf.size() - held, f)) > 0) {
    n += held; held = 0;
    if (to) { if (fwrite(buf.data(), 1, n, to) != n) die("appending " + path + " to the output failed"); continue; }
    size_t whole = 0;
    for (uint32_t bs; whole + 4 <= n && (memcpy(&bs, buf.data() + whole, 4), whole + 4 + (size_t)bs <= n);) whole += 4 + (size_t)bs;
    if (whole && fq_bam_write_records(bam, buf.data(), (int64_t)whole) != 0) die("appending " + path + " to the output failed");
    held = n - whole;
    if (held == buf.size()) die("appending " + path + " to the output failed: a record larger than the buffer");
    memmove(buf.data(), buf.data() + whole, held);
  }
  if (held) die("appending " + path + " to the output failed: the file ends inside a record");
  fclose(f);
  remove(path.c_str());
}

// The one column of the reference's output that is not reproduced: said loudly, or refused.
void unequal_lengths_notice(const Args &A, const fq_fastq_t *a, const fq_fastq_t *b, bool seen_on_device = false) {
  if (!seen_on_device && !(a && fq_fastq_unequal_lengths(a)) && !(b && fq_fastq_unequal_lengths(b))) return;
  const char *msg = "reads of unequal lengths: the reference prints the QUAL column of a read that follows a longer read in its read slot with that read's "
                    "tail behind it (an unterminated buffer: src/BwtMapper.cpp:549-558, libbwa/bwase.c:401; longer than SEQ, not valid SAM); here QUAL has "
                    "the read's own length -- every other column, and every QC file, is the reference's";
  if (A.strict) die(std::string("--strict_reference: ") + msg);
  fprintf(stderr, "WARNING - %s\n", msg);
}
fq_frontend_t *open_device_front_end(const Args &A, const std::string &f1, const std::string &f2, int device, int slot_mode, int stride) {
  if (A.host_reader || A.frac < 1.0) return nullptr;       // (--frac_samp: the reference's generator is walked record by record, on the host)
  fq_frontend_t *fe = nullptr;
  if (!A.bam_in.empty()) {
    std::vector<const char *> ids;
    for (const std::string &id : A.bam_rg) ids.push_back(id.c_str());
    const fq_bam_select_t sel{ids.data(), (int32_t)ids.size(), A.bam_oq ? 1 : 0};
    const bool tags = !ids.empty() || A.bam_oq;      // (neither option: the entries as they were, kernel for kernel)
    const int rc = A.collate ? (tags ? fq_frontend_open_bam_collate_select(device, A.bam_in.c_str(), A.o.batch_pairs, A.chunk_pairs, slot_mode, stride, A.collate_mem, &sel, &fe)
                                     : fq_frontend_open_bam_collate(device, A.bam_in.c_str(), A.o.batch_pairs, A.chunk_pairs, slot_mode, stride, A.collate_mem, &fe))
                             : (tags ? fq_frontend_open_bam_select(device, A.bam_in.c_str(), A.o.batch_pairs, A.chunk_pairs, slot_mode, stride, &sel, &fe)
                                     : fq_frontend_open_bam(device, A.bam_in.c_str(), A.o.batch_pairs, A.chunk_pairs, slot_mode, stride, &fe));
    mark("front end open");
    if (rc) die("--bam_in: cannot start the front end on device " + std::to_string(device) + " for " + A.bam_in + " (" + std::to_string(rc) + ")");
    return fe;
  }
  const int rc = fq_frontend_open(device, f1.c_str(), f2.empty() ? nullptr : f2.c_str(), A.o.batch_pairs, A.chunk_pairs, slot_mode, stride, &fe);
  mark("front end open");
  if (rc == FQ_EIO) return nullptr;                          // not a regular BGZF file: the host reader's
  if (rc) die("cannot start the front end on device " + std::to_string(device) + " (" + std::to_string(rc) + ")");
  return fe;
}
void front_end_notice(fq_frontend_t *fe, bool bam_tags = false) {
  fq_frontend_stats_t st;
  fq_frontend_stats(fe, &st);
  fprintf(stderr, "NOTICE - front end on the device: %lld pairs, %lld BGZF members (%lld left to the host's decoder), %.1f MB -> %.1f MB of text; inflate %.1f ms ; lines, records, keys, slots %.1f ms\n",
          (long long)st.pairs, (long long)st.members, (long long)st.refused, 1e-6 * (double)st.comp_bytes, 1e-6 * (double)st.text_bytes, st.ms_inflate, st.ms_tokenise);
  if (st.bam_records || st.ms_transcode > 0)
    fprintf(stderr, "NOTICE - BAM input on the device: %lld records (%lld skipped as secondary or supplementary), %lld repairs of the record chain; records -> text %.1f ms (starts %.1f, pairs %.1f, fill %.1f)\n",
            (long long)st.bam_records, (long long)st.bam_skipped, (long long)st.chain_repairs, st.ms_transcode, st.ms_bam_starts, st.ms_bam_pairs, st.ms_bam_fill);
  if (bam_tags)
    fprintf(stderr, "NOTICE - BAM input, auxiliary fields walked on the device: %lld records of other read groups left out, %lld records with their quality line from OQ; tag kernel %.1f ms\n",
            (long long)st.bam_unselected, (long long)st.bam_oq_records, st.ms_bam_tags);
  if (st.ms_bam_collate > 0 || st.bam_held_peak_records)
    fprintf(stderr, "NOTICE - BAM input collated on the device: at most %lld records (%.1f MB) waited for their mates; collation kernels %.1f ms\n",
            (long long)st.bam_held_peak_records, 1e-6 * (double)st.bam_held_peak_bytes, st.ms_bam_collate);
  if (st.bam_orphans) fprintf(stderr, "WARNING - BAM input: %lld records without a mate in the file (orphans) were left out\n", (long long)st.bam_orphans);
}


// One FASTQ pair (or one single-end file) through a device: an independent stream -- its own context (srand48, last_ii, position cache)
// and read slots, as PairEndMapper / SingleEndMapper set them up per call (src/BwtMapper.cpp:232-262).
// The front end of an input: on the device for BGZF files (fq_frontend_*: the host reads compressed bytes, everything per byte of text
// happens in HBM), on the host's threads for anything else (fq_fastq_*) -- and from the record on at which the device hands over (a
// record that is not four plain lines, a file that ends inside a record: fq_frontend_handover gives host readers standing exactly there).
// `ready`: called once the input's first chunk has been read and before anything needs the index, the QC consumer or the sink -- the
// one-device command line stages the index (about a second: the filter bitmaps are built on the device) on another thread meanwhile.
struct Stream {
  Args A;
  const bool se;
  fq_index_t *const &ix_ref;
  fq_qc_t *const &qc_ref;
  Sink &out;
  const std::function<void()> &ready;
  const int device;
  int slot_mode = 0, stride = 0, reader_threads = 1;
  long long num_read = 0, filtered = 0, unmapped = 0, order_checked_reads = 0;
  double qc_ms = 0, out_ms = 0, read_all_ms = 0, read_wait_ms = 0, align_ms = 0, read_ms = 0, pack_ms = 0;
  std::mutex tm_mu;                                  // (the consumers' timings, when they run on threads)
  bool started = false;                              // from then on: the index, the QC consumer, the sink
  fq_index_t *ix = nullptr;
  fq_qc_t *qc = nullptr;
  fq_ctx_t *ctx = nullptr, *ctx_a = nullptr, *ctx2 = nullptr;   // ctx: the context that holds the stream's state; ctx_a: the first one made; ctx2: the second of the device's part
  fq_frontend_t *fe = nullptr;
  bool unequal_on_device = false;
  std::thread th_qc, th_out;                         // the consumers of the device part's previous call
  std::unique_ptr<FastqReader> r[2];                 // the host readers

  Stream(const Args &A_, const std::pair<std::string, std::string> &input, fq_index_t *const &ix_, fq_qc_t *const &qc_, Sink &out_, const std::function<void()> &ready_, int device_)
      : A(A_), se(input.second.empty() || input.second == "Empty"), ix_ref(ix_), qc_ref(qc_), out(out_), ready(ready_), device(device_) {
    A.fq1 = input.first; A.fq2 = se ? "" : input.second;
    if (se) fprintf(stderr, "NOTICE - Processing Single End mapping\t%s\n", A.fq1.c_str());
    else fprintf(stderr, "NOTICE - Processing Pair End mapping\t%s\t%s\n", A.fq1.c_str(), A.fq2.c_str());
    // BwtMapper::SingleEndMapper (src/BwtMapper.cpp:1266-1407): its reader hands out fresh zeroed buffers (bwa_read_seq_with_hash, :350-475),
    // so neither bases nor name tails of earlier reads linger
    slot_mode = se ? FQ_FASTQ_SLOTS_FRESH : A.clean_names ? FQ_FASTQ_SLOTS_CLEAN_NAMES : FQ_FASTQ_SLOTS_REUSED;
    stride = row_stride(A, A.fq1, A.fq2);
    reader_threads = se ? A.pack_threads : std::max(1, A.pack_threads / 2);
  }
  void join_consumers() { if (th_qc.joinable()) th_qc.join(); if (th_out.joinable()) th_out.join(); }
  // The one refusal of a stream (refuse_run): consumers of the previous call that still run on their own threads are waited for first.
  // (Not for the consumers themselves, which may be those threads: their failures die() where they stand.)
  [[noreturn]] void fail(const std::string &m) { join_consumers(); refuse_run(out, m); }
  fq_ctx_t *new_context() {
    fq_ctx_t *c = nullptr;
    fq_opts_t o = A.o;
    o.single_end = se ? 1 : 0;
    const int rc = fq_ctx_create(ix, &o, (int32_t)A.chunk_pairs, &c);
    if (rc) fail("fq_ctx_create failed (" + std::to_string(rc) + "): option outside the supported range");
    attach_device_consumers(c, A, out.bam, qc);
    return c;
  }
  void start() {
    if (started) return;
    started = true;
    mark("first chunk there; waiting for the index");
    ready();
    mark("index ready");
    ix = ix_ref; qc = qc_ref;
    if (qc) fq_qc_begin_file(qc, A.fq1.c_str(), se ? A.fq1.c_str() : A.fq2.c_str());      // FileStatCollector(fq1[, fq2]): a single file is named twice
    ctx = ctx_a = new_context();
    mark("context created");
  }
  // the consumers of a call's records: StatCollector and the record writer (src/BwtMapper.cpp:2047-2050, 2075-2085).  The reference runs them
  // one after the other on its main thread; neither reads what the other writes here (each applies AddAlignment's contig-bridging mutation,
  // SURVEY Q10, to its own view of a record), so the device's part runs them side by side
  void consume_qc(fq_ctx_t *cx) {
    const auto t0 = Clock::now();
    if (qc && fq_qc_add_last(qc, cx)) die(std::string("QC consumer failed: ") + fq_qc_last_error(qc));
    std::lock_guard<std::mutex> lk(tm_mu);
    qc_ms += ms_since(t0);
  }
  void consume_out(fq_ctx_t *cx) {
    const auto t0 = Clock::now();
    fetch_records(A, cx, out);
    std::lock_guard<std::mutex> lk(tm_mu);
    out_ms += ms_since(t0);
  }
  void count(const fq_result_batch_t &res, long long n_reads) {
    num_read += n_reads; filtered += res.n_both_filtered; unmapped += res.n_both_unmapped;
    fprintf(stderr, se ? "NOTICE - %lld sequences are loaded.\n" : "NOTICE - %lld sequences are processed.\n", num_read);
  }

  // ---- the device's part of the stream: two contexts take the batches in turn, so that the consumers of one call's records work (on threads:
  //      they only move text and append) while the next call runs.  Ends with the input, or where the front end hands over to host readers.
  void device_loop() {
    fe = open_device_front_end(A, A.fq1, A.fq2, device, slot_mode, stride);
    if (!fe) return;
    fq_text_batch_t *tb_prev = nullptr;
    auto finish_prev = [&] {            // the previous call's consumers are done: its batch may be reused
      join_consumers();
      if (tb_prev) { fq_frontend_release(fe, tb_prev); tb_prev = nullptr; }
    };
    fq_ctx_t *cur = nullptr, *other = nullptr;
    for (;;) {
      const auto tr0 = Clock::now();
      fq_text_batch_t *tb = nullptr;
      const int64_t n = fq_frontend_next(fe, &tb);
      (started ? read_wait_ms : read_ms) += ms_since(tr0);
      if (n == FQ_EFALLBACK) {
        finish_prev();
        fq_fastq_t *h[2] = {nullptr, nullptr};
        if (const int rc = fq_frontend_handover(fe, reader_threads, h)) fail("the device front end could not hand " + A.fq1 + " over to the host reader (" + std::to_string(rc) + ")");
        r[0].reset(new FastqReader(A.fq1, h[0]));
        if (!se) r[1].reset(new FastqReader(A.fq2, h[1]));
        fprintf(stderr, "NOTICE - the FASTQ text from record %lld on is not four plain lines per record: read on by the host's reader\n", num_read / (se ? 1 : 2) + 1);
        break;
      }
      if (n < 0) fail(std::string(fq_frontend_last_error(fe)).empty() ? "the device front end failed (" + std::to_string(n) + ")" : fq_frontend_last_error(fe));
      if (n == 0) break;
      start();
      if (!cur) { cur = ctx; other = ctx2 = new_context(); }
      // the stream's order-dependent state -- drand48 stream, last_ii, (k,l) cache -- goes from the context of the last call to this one's
      else if (fq_ctx_state_move(cur, other)) fail("handing the stream's state from one context to the other failed");
      if (!se && order_check(A, order_checked_reads, (int)n, [&](int sb, int e) { const char *nm = fq_text_batch_first_name(tb, sb, e); return nm ? nm : ""; })) fail(kOutOfOrder);
      fq_result_batch_t res;
      const auto ta0 = Clock::now();
      if (fq_align_text(cur, tb, &res)) fail(std::string("fq_align_text failed: ") + fq_ctx_last_error(cur));
      align_ms += ms_since(ta0);
      mark("call done");
      finish_prev();
      mark("previous call's consumers done");
      count(res, se ? n : 2 * n);
      th_qc = std::thread([this, cur] { consume_qc(cur); });
      th_out = std::thread([this, cur] { consume_out(cur); });
      tb_prev = tb;
      std::swap(cur, other);            // (`other` now names the context of the call just made: the one whose state goes on)
    }
    finish_prev();
    if (other) ctx = other;             // the context that holds the stream's state (the host readers' part, if any, goes on with it)
    unequal_on_device = fq_frontend_unequal_lengths(fe) != 0;
    front_end_notice(fe, !A.bam_rg.empty() || A.bam_oq);
  }

  // ---- the host readers' part (all of it for files that are not BGZF): the next chunk is read and tokenised while the device aligns the
  //      current one; the consumers run on this thread, between the calls.  A single-end input is a chunk with one end.
  void host_loop() {
    const int ends = se ? 1 : 2;
    if (!fe) for (int e = 0; e < ends; ++e) r[e].reset(new FastqReader(e ? A.fq2 : A.fq1, reader_threads, A.o.batch_pairs, slot_mode, A.frac));
    if (!r[0]) return;                  // (the device's part was the whole input)
    FastqReader *const readers[2] = {r[0].get(), r[1].get()};
    Chunk bufs[2];
    for (Chunk &c : bufs) c.init(ends, A.chunk_pairs, stride);
    auto read_chunk = [&](int slot) { const auto t0 = Clock::now(); bufs[slot].fill(readers); read_all_ms += ms_since(t0); };
    { const auto t0 = Clock::now(); read_chunk(0); read_ms += ms_since(t0); }
    fq_packed_batch_t *pk = nullptr;    // packed-batch storage, reused from chunk to chunk (pinned once)
    for (int slot = 0;; slot ^= 1) {
      Chunk &c = bufs[slot];
      if (!c.error().empty()) fail(c.error());
      if (c.n == 0) break;
      start();
      if (!pk && fq_packed_create((int32_t)(se ? (A.chunk_pairs + 1) / 2 : A.chunk_pairs), stride, &pk)) fail("out of pinned host memory for the packed batch");
      std::thread prefetch;
      if (!c.last) prefetch = std::thread(read_chunk, slot ^ 1);          // next chunk while this one is on the device
      if (!se && order_check(A, order_checked_reads, c.n, [&](int sb, int e) { return c.first_name(sb, e, A.o.batch_pairs); })) fail(kOutOfOrder);
      c.squeeze();
      const fq_read_batch_t in = c.batch();
      fq_result_batch_t res;
      // the packed boundary: 24 bytes of filter keys per read cross PCIe, full rows only for the surviving pairs (or reads)
      const auto tp0 = Clock::now();
      const int rc = se ? fq_pack_single_reads_into(&in, A.pack_threads, pk) : fq_pack_reads_into(&in, A.pack_threads, pk);
      pack_ms += ms_since(tp0);
      if (rc) fail(std::string(se ? "fq_pack_single_reads_into" : "fq_pack_reads") + " failed (" + std::to_string(rc) + ")");
      const auto ta0 = Clock::now();
      if (fq_align_packed(ctx, pk, &res)) fail(std::string("fq_align_packed failed: ") + fq_ctx_last_error(ctx));
      align_ms += ms_since(ta0);
      consume_qc(ctx); consume_out(ctx); count(res, se ? c.n : 2LL * c.n);
      const auto tw0 = Clock::now();
      if (prefetch.joinable()) prefetch.join();
      read_wait_ms += ms_since(tw0);
      if (c.last) break;
    }
    if (pk) fq_packed_free(pk);
  }

  // ---- the closing notices; the stream's device objects are released beside whatever the caller does next
  void finish() {
    start();                            // (an input without a record: the consumers and the index are needed all the same)
    out.flush();
    unequal_lengths_notice(A, r[0] ? r[0]->h : nullptr, r[1] ? r[1]->h : nullptr, unequal_on_device);
    end_of_input_notices(se, num_read, filtered, unmapped);
    fq_stats_t st;
    fq_stats_get(ctx_a, &st);
    if (ctx2) {
      fq_stats_t s2;
      fq_stats_get(ctx2, &s2);
      for (int k = 0; k < 6; ++k) st.kernel_ms[k] += s2.kernel_ms[k];
      st.kernel_ms[FQ_K_EMIT] += s2.kernel_ms[FQ_K_EMIT]; st.kernel_ms[FQ_K_REC_KERNEL] += s2.kernel_ms[FQ_K_REC_KERNEL]; st.kernel_ms[FQ_K_MD_KERNEL] += s2.kernel_ms[FQ_K_MD_KERNEL];
      st.device_wait_ms += s2.device_wait_ms; st.host_cpu_ms += s2.host_cpu_ms;
      st.host_ms_total += s2.host_ms_total; st.wall_ms_total += s2.wall_ms_total;
    }
    fprintf(stderr, "NOTICE - device time (ms): prep %.1f width %.1f gap %.1f sa %.1f sw %.1f refine %.1f records %.1f md %.1f consumers' kernels %.1f ; host %.1f ; waited for the device %.1f ; calls' CPU %.1f ; wall %.1f\n", st.kernel_ms[0],
            st.kernel_ms[1], st.kernel_ms[2], st.kernel_ms[3], st.kernel_ms[4], st.kernel_ms[5], st.kernel_ms[FQ_K_REC_KERNEL], st.kernel_ms[FQ_K_MD_KERNEL], st.kernel_ms[FQ_K_EMIT], st.host_ms_total, st.device_wait_ms, st.host_cpu_ms, st.wall_ms_total);
    fprintf(stderr, "NOTICE - the calls of one context moved over PCIe (bytes per pair): to the device %.1f ; to the host %.1f (lists, counts, hit lists; with the consumers on the device their outputs leave it on streams of their own and are not in this figure)\n",
            st.pairs ? (double)st.h2d_bytes / (double)st.pairs : 0.0, st.pairs ? (double)st.d2h_bytes / (double)st.pairs : 0.0);
    fprintf(stderr, "NOTICE - consumers (ms): StatCollector %.1f ; %s writer %.1f ; first chunk read %.1f ; packing %.1f\n", qc_ms, A.sam_out ? "SAM" : "BAM", out_ms, read_ms, pack_ms);
    fprintf(stderr, "NOTICE - reading (ms): all chunks %.1f ; waited for %.1f ; alignment calls %.1f\n", read_all_ms, read_wait_ms, align_ms);
    if (qc) fq_qc_end_file(qc);
    mark("input done");
    // (the contexts' and the front end's gigabytes of device memory are given back beside whatever the caller does next -- the next input's first
    //  chunk, the QC files: 80 ms of a 67 M-pair run)
    fq_ctx_t *a = ctx_a, *b = ctx2;
    fq_frontend_t *f = fe;
    release_later([a, b, f] {
      fq_ctx_destroy(a);
      mark("first context released");
      if (b) fq_ctx_destroy(b);
      if (f) fq_frontend_close(f);
      mark("contexts and front end released");
    });
  }
};
void align_input(const Args &A, const std::pair<std::string, std::string> &input, fq_index_t *const &ix, fq_qc_t *const &qc, Sink &out, const std::function<void()> &ready, int device) {
  Stream s(A, input, ix, qc, out, ready, device);
  s.device_loop();
  s.host_loop();
  s.finish();
}

// one worker per entry of --devices: its own copy of the index on its device, its own consumers
struct Worker { int device = 0; fq_index_t *ix = nullptr; fq_qc_t *qc = nullptr; fq_bam_t *bam = nullptr; std::thread th; };

// ---- ONE FASTQ pair over several devices: chunks of whole reference batches are dealt round-robin; every device runs filter,
//      search and SA walks of its chunk at once; the stream's order-dependent state -- the drand48 stream (srand48 once per FASTQ pair,
//      src/BwtMapper.cpp:1817), last_ii (:780-781), the (k,l) cache (:815-843) -- goes from the context that owns chunk b to the one that
//      owns b + 1 around the short serial part of each call (fq_ctx_set_serial_hooks / fq_ctx_state_export / _import).  The records come
//      out in chunk order through one writer; every chunk's StatCollector state is a segment, merged in order.
struct ShardRun {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<Chunk> slots;
  long long n_chunks = -1;                 // known once the reader has seen the end
  long long token_of = -1;                 // the stream's state after chunk token_of
  std::vector<char> token;
  struct Result { std::vector<char> records, qc; long long pairs = 0, filtered = 0, unmapped = 0; };   // records: SAM text, or BAM records as bytes
  std::map<long long, Result> results;
  // a refusal (a reader's error, a call that fails on chunk b): the writer still emits every chunk before it, then the run dies with `error`
  long long fail_at = -1;
  std::string error;
  void refuse(long long b, const std::string &m) {
    { std::lock_guard<std::mutex> lk(mu); if (fail_at < 0 || b < fail_at) { fail_at = b; error = m; } }
    cv.notify_all();
  }
};
struct ShardHook { ShardRun *run; fq_ctx_t *ctx; long long b; };
void shard_before(void *u) {
  ShardHook *h = (ShardHook *)u;
  if (h->b == 0) return;
  std::unique_lock<std::mutex> lk(h->run->mu);
  h->run->cv.wait(lk, [&] { return h->run->token_of == h->b - 1; });
  if (fq_ctx_state_import(h->ctx, h->run->token.data(), (int64_t)h->run->token.size())) fq_ctx_mark_stream_broken(h->ctx);
}
void shard_after(void *u) {
  ShardHook *h = (ShardHook *)u;
  const int64_t need = fq_ctx_state_export(h->ctx, nullptr, 0);
  std::vector<char> t((size_t)std::max<int64_t>(need, 0));
  if (need > 0) fq_ctx_state_export(h->ctx, t.data(), need);
  { std::lock_guard<std::mutex> lk(h->run->mu); h->run->token.swap(t); h->run->token_of = h->b; }
  h->run->cv.notify_all();
}
void align_pair_sharded(const Args &A, const std::pair<std::string, std::string> &input, std::vector<Worker> &wk, Sink &out, fq_qc_t *qc) {
  const size_t NW = wk.size();
  fprintf(stderr, "NOTICE - Processing Pair End mapping on %zu devices\t%s\t%s\n", NW, input.first.c_str(), input.second.c_str());
  const int slot_mode = A.clean_names ? FQ_FASTQ_SLOTS_CLEAN_NAMES : FQ_FASTQ_SLOTS_REUSED;
  FastqReader r1(input.first, std::max(1, A.pack_threads / 2), A.o.batch_pairs, slot_mode, A.frac), r2(input.second, std::max(1, A.pack_threads / 2), A.o.batch_pairs, slot_mode, A.frac);
  const int stride = row_stride(A, input.first, input.second);
  ShardRun R;
  R.slots.resize(NW + 1);
  for (Chunk &c : R.slots) c.init(2, A.chunk_pairs, stride);
  if (qc) fq_qc_begin_file(qc, input.first.c_str(), input.second.c_str());
  // the reader: chunks in file order into free slots
  std::thread reader([&] {
    FastqReader *const readers[2] = {&r1, &r2};
    long long order_checked_reads = 0;
    for (long long b = 0;; ++b) {
      Chunk *c = nullptr;
      {
        std::unique_lock<std::mutex> lk(R.mu);
        R.cv.wait(lk, [&] { for (auto &s : R.slots) if (s.index == -1) { c = &s; return true; } return false; });
        c->index = -2;
      }
      c->fill(readers);
      if (!c->error().empty()) { R.refuse(b, c->error()); return; }
      if (order_check(A, order_checked_reads, c->n, [&](int sb, int e) { return c->first_name(sb, e, A.o.batch_pairs); })) { R.refuse(b, kOutOfOrder); return; }
      c->squeeze();
      const bool last = c->last;
      {
        std::lock_guard<std::mutex> lk(R.mu);
        c->index = c->n ? b : -1;
        if (last) R.n_chunks = c->n ? b + 1 : b;
      }
      R.cv.notify_all();
      if (last) break;
    }
  });
  // the workers: chunk b goes to device b mod NW
  auto work = [&](size_t w) {
    Worker &K = wk[w];
    fq_ctx_t *ctx = nullptr;
    if (fq_ctx_create(K.ix, &A.o, (int32_t)A.chunk_pairs, &ctx)) die("fq_ctx_create failed: option outside the supported range");
    fq_packed_batch_t *pk = nullptr;
    if (fq_packed_create((int32_t)A.chunk_pairs, stride, &pk)) die("out of pinned host memory for the packed batch");
    if (K.qc) { fq_qc_begin_file(K.qc, input.first.c_str(), input.second.c_str()); if (fq_qc_state_reset(K.qc)) die("QC consumer: cannot start a segment"); }
    attach_device_consumers(ctx, A, K.bam, K.qc);
    for (long long b = (long long)w;; b += (long long)NW) {
      Chunk *c = nullptr;
      {
        std::unique_lock<std::mutex> lk(R.mu);
        R.cv.wait(lk, [&] { for (auto &s : R.slots) if (s.index == b) { c = &s; return true; } return (R.n_chunks >= 0 && b >= R.n_chunks) || R.fail_at >= 0; });
        if (!c) break;
      }
      const fq_read_batch_t in = c->batch();
      if (fq_pack_reads_into(&in, std::max(1, A.pack_threads / (int)NW), pk)) die("fq_pack_reads failed");
      ShardHook hook{&R, ctx, b};
      fq_ctx_set_serial_hooks(ctx, shard_before, shard_after, &hook);
      fq_result_batch_t res;
      if (fq_align_packed(ctx, pk, &res)) { R.refuse(b, std::string("fq_align_packed failed on device ") + std::to_string(K.device) + ": " + fq_ctx_last_error(ctx)); return; }
      ShardRun::Result got;
      got.pairs = c->n; got.filtered = res.n_both_filtered; got.unmapped = res.n_both_unmapped;
      if (K.qc) {
        if (fq_qc_add_last(K.qc, ctx)) die(std::string("QC consumer failed: ") + fq_qc_last_error(K.qc));
        qc_export_segment(K.qc, got.qc);
      }
      Sink mem;
      mem.bam = K.bam; mem.mem = &got.records; mem.what = "a chunk's records";
      fetch_records(A, ctx, mem);
      {
        std::lock_guard<std::mutex> lk(R.mu);
        c->index = -1;                       // the chunk's rows are free again (the consumers above were the last to read them)
        R.results.emplace(b, std::move(got));
      }
      R.cv.notify_all();
    }
    fq_ctx_destroy(ctx);
    fq_packed_free(pk);
  };
  std::vector<std::thread> th;
  for (size_t w = 0; w < NW; ++w) th.emplace_back(work, w);
  // the writer: results in chunk order
  long long num_read = 0, filtered = 0, unmapped = 0;
  for (long long b = 0;; ++b) {
    ShardRun::Result res;
    {
      std::unique_lock<std::mutex> lk(R.mu);
      R.cv.wait(lk, [&] { return R.results.count(b) || (R.n_chunks >= 0 && b >= R.n_chunks) || (R.fail_at >= 0 && b >= R.fail_at); });
      auto it = R.results.find(b);
      if (it == R.results.end() || (R.fail_at >= 0 && b >= R.fail_at)) break;
      res = std::move(it->second);
      R.results.erase(it);
    }
    out.records(res.records);
    if (qc && fq_qc_merge(qc, res.qc.data(), (int64_t)res.qc.size())) die(std::string("QC consumer: merge failed: ") + fq_qc_last_error(qc));
    num_read += 2 * res.pairs; filtered += res.filtered; unmapped += res.unmapped;
    fprintf(stderr, "NOTICE - %lld sequences are processed.\n", num_read);
  }
  {   // a refused run ends here, behind the records of the chunks before the refusal (threads that wait for a state that never comes end with the process)
    std::string err;
    { std::lock_guard<std::mutex> lk(R.mu); if (R.fail_at >= 0) err = R.error; }
    if (!err.empty()) refuse_run(out, err);
  }
  reader.join();
  for (auto &t : th) t.join();
  out.flush();
  unequal_lengths_notice(A, r1.h, r2.h);
  end_of_input_notices(false, num_read, filtered, unmapped);
  if (qc) fq_qc_end_file(qc);
}


// ---- a run: the options, its inputs, what the index says about itself, a worker per device
struct Run {
  Args A;
  std::vector<std::pair<std::string, std::string>> inputs;
  std::string pre, fai;          // <index_prefix>.FASTQuick.fa ; the original reference's .fai
  fq_qc_opts_t qo;
  bool have_qc = false;          // the index carries its .SelectedSite.vcf: the QC files are written
  std::vector<int> devices;
  std::vector<Worker> wk;
  std::string worker_prefix(size_t w) const { return A.out_prefix + ".worker" + std::to_string(w); }
};
// --bam_in: what it cannot be combined with, and the host's look at the file (fq_bam_probe): paired or single-end, the rows' width
bool probe_bam_input(Args &A) {
  // BAM input runs through the device front end alone: the flags below take host FASTQ readers, or shard over them (a host-side BAM reader is not built)
  if (!A.fq1.empty() || !A.fq2.empty()) die("--bam_in is an input of its own: it cannot be combined with --fastq_1 / --fastq_2");
  if (!A.fq_list.empty()) die("--bam_in cannot be combined with --fq_list (a list of BAM files is not supported)");
  if (A.host_reader) die("--bam_in cannot be combined with --host_reader (BAM records are read on the device only)");
  if (A.frac < 1.0) die("--bam_in cannot be combined with --frac_samp below 1 (sampling walks the records on the host)");
  if (!A.devices.empty() && parse_devices(A.devices).size() > 1) die("--bam_in cannot be combined with --devices naming more than one device (sharding takes host readers)");
  fq_bam_probe_t pr;
  if (!A.bam_rg.empty()) {                       // every wanted ID is one of the header's @RG lines: said before any device work
    int32_t n = 0;
    int64_t nb = 0;
    int rc = fq_bam_read_groups(A.bam_in.c_str(), nullptr, 0, &n, &nb);
    std::vector<char> buf((size_t)nb + 1);
    if (rc == FQ_ELIMIT) rc = fq_bam_read_groups(A.bam_in.c_str(), buf.data(), nb, &n, &nb);
    if (rc) { if (fq_bam_probe(A.bam_in.c_str(), &pr)) die(std::string("--bam_in: ") + pr.error); die("--bam_in: the header's @RG lines cannot be read"); }
    std::vector<std::string> have;
    for (const char *q = buf.data(); (int32_t)have.size() < n; q += have.back().size() + 1) have.emplace_back(q);
    std::string list;
    for (const std::string &h : have) list += (list.empty() ? "" : ", ") + h;
    for (const std::string &id : A.bam_rg)
      if (std::find(have.begin(), have.end(), id) == have.end())
        die("--bam_rg " + id + ": " + A.bam_in + " has no @RG line with this ID; its header holds " + (have.empty() ? std::string("no @RG line") : std::to_string(have.size()) + ": " + list));
  }
  std::vector<const char *> ids;
  for (const std::string &id : A.bam_rg) ids.push_back(id.c_str());
  const fq_bam_select_t sel{ids.data(), (int32_t)ids.size(), A.bam_oq ? 1 : 0};
  if (ids.empty() ? fq_bam_probe(A.bam_in.c_str(), &pr) : fq_bam_probe_select(A.bam_in.c_str(), &sel, &pr)) die(std::string("--bam_in: ") + pr.error);
  A.bam_l_seq = pr.first_l_seq;
  if (!strcmp(pr.sort_order, "coordinate") && !A.collate) fprintf(stderr, "NOTICE - %s says SO:coordinate: mates must be adjacent (collate the file by name first)\n", A.bam_in.c_str());
  return pr.paired != 0;
}
// --fq_list: one FASTQ pair per line, '#' lines skipped (src/BwtMapper.cpp:232-262); every pair is an independent stream
// (its own srand48, last_ii, position cache and read slots: PairEndMapper sets them up per call), all into one output
std::vector<std::pair<std::string, std::string>> read_inputs(const Args &A, bool bam_paired) {
  std::vector<std::pair<std::string, std::string>> inputs;
  if (!A.bam_in.empty()) { inputs.emplace_back(A.bam_in, bam_paired ? A.bam_in : ""); return inputs; }
  if (A.fq_list.empty()) {
    if (A.fq1.empty()) die("--fastq_1 (and --fastq_2 for paired-end reads), or --fq_list, is required");
    inputs.emplace_back(A.fq1, A.fq2);
    return inputs;
  }
  FILE *fl = fopen(A.fq_list.c_str(), "r");
  if (!fl) die("Open file " + A.fq_list + " failed");
  char line[8192];
  while (fgets(line, sizeof line, fl)) {
    if (line[0] == '#') continue;
    char a[4096] = "", b[4096] = "";
    const int got = sscanf(line, "%4095s %4095s", a, b);
    if (got < 1) continue;
    inputs.emplace_back(a, got < 2 ? "" : b);      // one column: single-end (src/BwtMapper.cpp:255-262)
  }
  fclose(fl);
  return inputs;
}
// <index>.param: REFERENCE_PATH, TARGET_REGION_PATH, DBSNP_VCF_PATH, NUM_VAR_LONG, NUM_VAR_SHORT, SHORT_FLANK_LENGTH, LONG_FLANK_LENGTH;
// the genome's size from the original reference's .fai / .amb; whether the index carries what the QC consumer needs
void read_index_params(Run &R) {
  const Args &A = R.A;
  R.pre = A.index_prefix + ".FASTQuick.fa";
  fq_qc_default_opts(&R.qo);
  R.qo.read_len = A.read_len; R.qo.cal_dup = A.cal_dup ? 1 : 0;
  std::string ref_path;
  FILE *fp = fopen((R.pre + ".param").c_str(), "r");
  char key[256], val[4096];
  while (fp && fscanf(fp, "%255s %4095s", key, val) == 2) {
    if (!strcmp(key, "REFERENCE_PATH")) ref_path = val;
    else if (!strcmp(key, "SHORT_FLANK_LENGTH")) R.qo.flank_len = atoi(val);
    else if (!strcmp(key, "LONG_FLANK_LENGTH")) R.qo.flank_long_len = atoi(val);
  }
  if (fp) fclose(fp);
  if (!ref_path.empty()) {   // BwtIndexer::LoadContigSize (src/BwtIndexer.cpp:764-802): sums of column 2 of the .fai and of EVERY line of the .amb
    char line[8192], a[4096], b[4096];
    if (FILE *ff = fopen((ref_path + ".fai").c_str(), "r")) { while (fgets(line, sizeof line, ff)) if (sscanf(line, "%4095s %4095s", a, b) == 2) R.qo.genome_size += atoi(b); fclose(ff); }
    if (FILE *fa = fopen((ref_path + ".amb").c_str(), "r")) { while (fgets(line, sizeof line, fa)) if (sscanf(line, "%4095s %4095s", a, b) == 2) R.qo.genome_n_size += atoi(b); fclose(fa); }
  }
  struct stat sb;
  R.have_qc = stat((R.pre + ".SelectedSite.vcf").c_str(), &sb) == 0;
  if (!R.have_qc) fprintf(stderr, "NOTICE - %s.SelectedSite.vcf not found: the QC files are not written\n", R.pre.c_str());
  if (!A.sam_out && ref_path.empty()) die("BAM output needs the original reference's .fai: " + R.pre + ".param (REFERENCE_PATH) is missing; or pass --sam_out");
  R.fai = ref_path + ".fai";
}
// The devices of the run, a worker each.  True: one FASTQ pair is sharded over several devices.
bool pick_devices(Run &R) {
  const Args &A = R.A;
  R.devices = A.devices.empty() ? std::vector<int>{A.device} : parse_devices(A.devices);
  const bool shard_one_pair = R.devices.size() > 1 && R.inputs.size() == 1 && !R.inputs[0].second.empty() && R.inputs[0].second != "Empty";
  if (!shard_one_pair && R.devices.size() > R.inputs.size()) R.devices.resize(std::max<size_t>(1, R.inputs.size()));   // (a worker per FASTQ pair at most)
  // every ordinal is checked before anything is started (a worker that fails to load its index would take the run down half-way)
  const int n_dev = fq_device_count();
  if (n_dev <= 0) die("no HIP device is visible; there is no CPU fallback");
  for (int d : R.devices) if (d >= n_dev) die("device " + std::to_string(d) + " does not exist (" + std::to_string(n_dev) + " visible)");
  mark("devices counted");
  R.wk = std::vector<Worker>(R.devices.size());
  return shard_one_pair;
}
// The writer of the run's BAM file: <out_prefix>.bam in input order, or with --sorted_bam <out_prefix>.sorted.bam in coordinate order with its index.
int create_bam_file(const Args &A, const char *path, const fq_index_t *ix, const std::string &fai, const fq_qc_opts_t *qo, fq_bam_t **out) {
  const int rc = A.sorted_bam ? fq_bam_create_sorted(ix, fai.c_str(), path, A.rg.c_str(), qo, A.sort_mem, out) : fq_bam_create(ix, fai.c_str(), path, A.rg.c_str(), qo, out);
  if (!rc && A.bam_deflate >= 0 && fq_bam_set_deflate(*out, A.bam_deflate)) die("--bam_deflate: the writer refused the mode");
  return rc;
}
// ... and its close; a sorted writer says what it held and where the close's time went
bool close_bam_file(const Args &A, fq_bam_t *bam) {
  fq_bam_sort_stats_t st{};
  fq_bam_deflate_stats_t zs{};
  if (A.sorted_bam) fq_bam_sort_stats_at_close(bam, &st);
  fq_bam_deflate_stats_at_close(bam, &zs);
  if (fq_bam_close(bam)) return false;
  if (zs.mode == FQ_DEFLATE_DYNAMIC)
    fprintf(stderr, "NOTICE - BAM writer: deflate mode dynamic (block type chosen per member): %lld of the device's members took dynamic Huffman tables, %lld the fixed code\n", (long long)zs.members_dynamic, (long long)zs.members_fixed);
  else fprintf(stderr, "NOTICE - BAM writer: deflate mode fixed (one fixed-Huffman block per member of the device)\n");
  if (A.sorted_bam) {
    fprintf(stderr, "NOTICE - sorted BAM: %lld records in %lld runs (%lld sorted on the device inside their calls, %lld spilled to files); keys of %d bits\n", (long long)st.records, (long long)st.runs,
            (long long)st.device_sorted_runs, (long long)st.spilled_runs, st.key_bits);
    fprintf(stderr, "NOTICE - sorted BAM: entries and sort kernels %.3f ms (the calls' runs and the close's key sort) ; gather kernels %.3f ms (the calls' runs) ; close %.3f s (key sort %.3f ; assembly %.3f ; compression and writing %.3f ; index %.3f)\n", st.sort_kernel_ms,
            st.gather_kernel_ms, st.close_sec, st.close_sort_sec, st.close_assemble_sec, st.close_compress_sec, st.close_index_sec);
  }
  return true;
}
// Worker w: the index onto its device, its QC consumer (files under qc_prefix) and its BAM writer (bam_path null: a formatter without a file).
void open_worker(Run &R, size_t w, const std::string &qc_prefix, const char *bam_path) {
  const Args &A = R.A;
  Worker &K = R.wk[w];
  K.device = R.devices[w];
  const auto t_ix0 = Clock::now();
  int rc = fq_index_load(R.pre.c_str(), K.device, &K.ix);
  fprintf(stderr, "NOTICE - index staged on device %d in %.1f ms\n", K.device, ms_since(t_ix0));
  if (rc) die("cannot load index " + R.pre + " onto HIP device " + std::to_string(K.device) + " (" + std::to_string(rc) + "); there is no CPU fallback");
  if (R.have_qc) {
    if (qc_prefix != A.out_prefix) tmp_file(qc_prefix + ".InsertSizeTable");
    rc = fq_qc_create(K.ix, R.pre.c_str(), qc_prefix.c_str(), &R.qo, &K.qc);
    if (rc) die("cannot set up the QC consumer from " + R.pre + ".SelectedSite.vcf / .dbSNP.subset.vcf / .gc (" + std::to_string(rc) + ")");
    mark("QC consumer set up");
  }
  if (!A.sam_out) {
    rc = bam_path ? create_bam_file(A, bam_path, K.ix, R.fai, &R.qo, &K.bam) : fq_bam_create(K.ix, R.fai.c_str(), nullptr, A.rg.c_str(), &R.qo, &K.bam);
    if (rc) die("cannot open " + std::string(bam_path ? bam_path : "a BAM formatter") + " / " + R.fai + " (" + std::to_string(rc) + ")");
    mark("BAM writer set up");
  }
}
// The outputs of a run over several devices, which its main thread writes from what the workers produced: the SAM header on stdout or the BAM
// file, and the QC consumer that the workers' segments are merged into.
struct Merged { Sink out; fq_qc_t *qc = nullptr; };
Merged open_merged(Run &R) {
  const Args &A = R.A;
  Merged M;
  M.out = direct_sink(A);
  if (A.sam_out) write_sam_header(R.wk[0].ix);
  else if (create_bam_file(A, A.bam_file().c_str(), R.wk[0].ix, R.fai, &R.qo, &M.out.bam)) die("cannot open " + A.bam_file() + " / " + R.fai);
  if (R.have_qc && fq_qc_create(R.wk[0].ix, R.pre.c_str(), A.out_prefix.c_str(), &R.qo, &M.qc)) die("cannot set up the QC consumer");
  return M;
}
// `align --popcon_svd P`: the estimate of `pop+con` straight from the run.  The marker pileups the QC consumer holds (what it has just printed as O.Pileup) go to the
// estimator in memory: a base equal to the .bed's ref allele becomes '.' or ',' by strand, entries with a mapping quality below 13 or a base quality below 2 are left out
// (min_mq and min_baseQ of the reference's BAM route, SimplePileupViewer.cpp:678-679).  No BAQ and no handling of overlapping mates: the result is that of
// `pop+con --PileupFile` on the pileup converted the same way.  Writes O.selfSM and O.Ancestry and appends its line to O.Summary.
struct PopconFeed { fq_popcon_t *p; std::vector<int32_t> marker; std::vector<char> base, qual; };
void popcon_after_qc(const Args &A, fq_qc_t *qc, int device) {
  if (A.popcon_svd.empty()) return;
  if (!qc) die("--popcon_svd reads the QC consumer's marker pileups: the index needs its .SelectedSite.vcf");
  if (!fq_popcon_create) die("--popcon_svd: this build of the library has no estimator");
  fq_popcon_opts_t o;
  fq_popcon_default_opts(&o);
  o.num_pc = A.popcon_numpc;
  o.within_ancestry = A.popcon_within;
  o.device = device;
  PopconFeed F;
  if (fq_popcon_create(A.popcon_svd.c_str(), nullptr, nullptr, nullptr, &o, &F.p)) die(std::string("--popcon_svd: ") + fq_popcon_last_error(nullptr));
  const int rc = fq_qc_piles(qc, [](void *user, const char *chrom, int32_t pos, int64_t n, const char *bases, const char *quals, const uint8_t *maq, const int8_t *base_qual) -> int {
    PopconFeed &f = *(PopconFeed *)user;
    const int32_t row = fq_popcon_marker_index(f.p, chrom, pos);
    if (row < 0) return 0;
    char ref = 0;
    fq_popcon_marker_alleles(f.p, row, &ref, nullptr);
    for (int64_t t = 0; t < n; ++t) {
      if (maq[t] < 13 || base_qual[t] < 2) continue;
      char c = bases[t];
      if (toupper((unsigned char)c) == toupper((unsigned char)ref)) c = isupper((unsigned char)c) ? '.' : ',';
      f.marker.push_back(row); f.base.push_back(c); f.qual.push_back(quals[t]);
    }
    return 0;
  }, &F);
  if (rc) die("--popcon_svd: walking the marker pileups failed");
  auto fail = [&](const char *what) { const std::string m = std::string("--popcon_svd: ") + what + ": " + fq_popcon_last_error(F.p); die(m); };
  if (fq_popcon_set_pileup_arrays(F.p, F.marker.data(), F.base.data(), F.qual.data(), (int64_t)F.marker.size())) fail("pileup");
  if (fq_popcon_run(F.p)) fail("estimate");
  if (fq_popcon_write(F.p, A.out_prefix.c_str())) fail("output");
  fq_popcon_destroy(F.p);
  mark("contamination and ancestry estimated");
}
void close_merged(Run &R, Merged &M) {   // ... and the workers' objects go
  M.out.flush();
  if (M.out.bam && !close_bam_file(R.A, M.out.bam)) die("closing " + R.A.bam_file() + " failed");
  if (M.qc) {
    if (fq_qc_write(M.qc)) die("writing the QC files failed");
    popcon_after_qc(R.A, M.qc, R.devices[0]);
    fq_qc_destroy(M.qc);
  }
  release_join();
  for (size_t w = 0; w < R.wk.size(); ++w) {
    Worker &K = R.wk[w];
    if (K.bam) fq_bam_close(K.bam);
    if (K.qc) { fq_qc_destroy(K.qc); remove((R.worker_prefix(w) + ".InsertSizeTable").c_str()); }
    fq_index_destroy(K.ix);
  }
}
Args worker_args(const Run &R) {   // the host's CPUs are shared by the workers
  Args AW = R.A;
  if (AW.o.host_threads <= 0) AW.o.host_threads = std::max(2, std::min(16, 2 * fq_host_cpus() / (int)R.wk.size()));
  return AW;
}

// ---- one device: the records go out as they are produced.  The index is staged, and the consumers are set up, while the first input's
//      first chunk is read and tokenised.
void run_one_device(Run &R) {
  const Args &A = R.A;
  Worker &K = R.wk[0];
  const std::string bam_path = A.bam_file();
  std::thread opener([&] { open_worker(R, 0, A.out_prefix, A.sam_out ? nullptr : bam_path.c_str()); });
  Sink out = direct_sink(A);
  bool opened = false;
  const std::function<void()> ready = [&] {
    if (opened) return;
    opened = true;
    opener.join();
    out.bam = K.bam;
    if (A.sam_out) write_sam_header(K.ix);
  };
  for (const auto &input : R.inputs) align_input(A, input, K.ix, K.qc, out, ready, R.devices[0]);   // (not K.device: the opener thread is still writing K)
  ready();
  // (the BAM file's last blocks and its close beside the QC files' writing: a third of a second of a deep run's tail)
  bool bam_bad = false;
  std::thread closer;
  if (K.bam) closer = std::thread([&] { bam_bad = !close_bam_file(A, K.bam); mark("BAM file closed"); });
  const bool qc_bad = K.qc && fq_qc_write(K.qc) != 0;
  if (closer.joinable()) closer.join();
  if (bam_bad) die("closing " + A.bam_file() + " failed");
  if (qc_bad) die("writing the QC files failed");
  mark("QC files written");
  popcon_after_qc(A, K.qc, R.devices[0]);
  if (K.qc) { fq_qc_t *qc = K.qc; release_later([qc] { fq_qc_destroy(qc); mark("QC consumer released"); }); }      // (beside the contexts' release)
  release_join();
  fq_index_destroy(K.ix);
  mark("index released");
}
// ---- one FASTQ pair over several devices: chunks dealt round-robin, the stream's state handed from context to context (align_pair_sharded)
void run_sharded_pair(Run &R) {
  std::vector<std::thread> opn;
  for (size_t w = 0; w < R.wk.size(); ++w) opn.emplace_back([&R, w] { open_worker(R, w, R.worker_prefix(w), nullptr); });
  for (auto &t : opn) t.join();
  Merged M = open_merged(R);
  align_pair_sharded(worker_args(R), R.inputs[0], R.wk, M.out, M.qc);
  close_merged(R, M);
}
// ---- several devices: the lines of --fq_list are dealt over them (the next free worker takes the next pair); every pair's records go
//      to part files of its own and its StatCollector state to a segment (fq_qc_state_export); the main thread puts the parts behind
//      each other and merges the segments (fq_qc_merge) in input order -- the files of the one-device run (src/BwtMapper.cpp:232-262,
//      src/StatCollector.h:46-62: one StatCollector over all pairs of the list)
void run_list_over_devices(Run &R) {
  const Args &A = R.A;
  const size_t n_in = R.inputs.size();
  std::vector<std::vector<char>> segment(n_in);
  std::atomic<size_t> next{0};
  Args AW = worker_args(R);
  AW.pack_threads = std::max(1, A.pack_threads / (int)R.wk.size());
  auto part = [&](size_t i) { return A.out_prefix + ".part" + std::to_string(i) + (A.sam_out ? ".sam" : ".bamrec"); };
  auto work = [&](size_t w) {
    open_worker(R, w, R.worker_prefix(w), nullptr);
    Worker &K = R.wk[w];
    if (K.qc && fq_qc_state_reset(K.qc)) die("QC consumer: cannot start a segment");
    for (size_t i; (i = next.fetch_add(1)) < n_in;) {
      Sink out;
      out.bam = K.bam;
      out.what = part(i);
      tmp_file(out.what);
      FILE *f = fopen(out.what.c_str(), "wb");
      if (!f) die("cannot create " + out.what);
      (A.sam_out ? out.sam_fp : out.bam_fp) = f;
      fprintf(stderr, "NOTICE - device %d takes line %zu of the list\n", K.device, i + 1);
      align_input(AW, R.inputs[i], K.ix, K.qc, out, [] {}, K.device);
      if (fclose(f)) die("writing " + out.what + " failed");
      if (K.qc) qc_export_segment(K.qc, segment[i]);
    }
  };
  for (size_t w = 0; w < R.wk.size(); ++w) R.wk[w].th = std::thread(work, w);
  for (auto &K : R.wk) K.th.join();
  Merged M = open_merged(R);   // the output, in input order
  for (size_t i = 0; i < n_in; ++i) {
    append_file(part(i), M.out.sam_fp, M.out.bam);
    if (M.qc && fq_qc_merge(M.qc, segment[i].data(), (int64_t)segment[i].size())) die(std::string("QC consumer: merge failed: ") + fq_qc_last_error(M.qc));
  }
  close_merged(R, M);
}
}  // namespace

// `FASTQuick pop+con` (VerifyBamID/vb2Main.cpp runVB2): flags of the reference's names and meanings
static int popcon_main(int argc, char **argv) {
  if (!fq_popcon_create) die("pop+con: this build of the library has no estimator");
  fq_popcon_opts_t o;
  fq_popcon_default_opts(&o);
  std::string pileup = "Empty", svd = "Empty", out = "result", ud = "Empty", mu = "Empty", bed = "Empty", known_af;
  for (int i = 2; i < argc; ++i) {
    const std::string f = argv[i];
    auto need = [&]() -> const char * { if (i + 1 >= argc) die("missing value for " + f); return argv[++i]; };
    if (f == "--PileupFile") pileup = need();
    else if (f == "--SVDPrefix") svd = need();
    else if (f == "--Output") out = need();
    else if (f == "--NumPC") o.num_pc = atoi(need());
    else if (f == "--WithinAncestry") o.within_ancestry = 1;
    else if (f == "--DisableSanityCheck") o.disable_sanity_check = 1;
    else if (f == "--FixPC") {   // PC1:PC2:.. (vb2Main.cpp:165-182)
      fprintf(stderr, "NOTICE - you specified --fixPC, this will overide dynamic estimation of PCs\n");
      const std::string v = need();
      size_t a = 0;
      int n = 0;
      while (a <= v.size()) {
        const size_t b = std::min(v.find(':', a), v.size());
        if (n < 8) o.fix_pc_values[n] = atof(v.substr(a, b - a).c_str());
        ++n;
        a = b + 1;
      }
      o.fix_pc = n;
    }
    else if (f == "--FixAlpha") { o.fix_alpha_value = atof(need()); o.fix_alpha = 1; }
    else if (f == "--KnownAF") known_af = need();
    else if (f == "--Epsilon") o.epsilon = atof(need());
    else if (f == "--UDPath") ud = need();
    else if (f == "--MeanPath") mu = need();
    else if (f == "--BedPath") bed = need();
    else if (f == "--host_eval") o.host_eval = 1;
    else if (f == "--device") o.device = atoi(need());
    else if (f == "--Seed" || f == "--NumThread" || f == "--Reference") { need(); fprintf(stderr, "NOTICE - %s is accepted and ignored: the estimate draws no random number, sizes its own threads and reads no reference file\n", f.c_str()); }
    else if (f == "--BamFile") die("--BamFile is not supported (the BAM route needs BAQ and htslib's overlap handling): give the pileup with --PileupFile");
    else if (f == "--RefVCF") die("--RefVCF is not supported here (`FASTQuick_amd svd --RefVCF` makes the SVD files): give their prefix with --SVDPrefix, and the pileup with --PileupFile");
    else die("unknown option " + f);
  }
  if (o.num_pc > 4) die("--NumPC only permits as large as 4 PCs when using SVD files in ${verifybamID}/resource/ directory!");
  if (o.fix_pc) {
    if (o.fix_pc < o.num_pc) die("parameter --fixPC provided smaller dimension than parameter --numPC");
    if (o.fix_pc > o.num_pc) fprintf(stderr, "WARNING - parameter --fixPC provided larger dimension than parameter --numPC and hence will be truncated\n");
    o.fix_pc = 1;
  } else if (o.fix_alpha && fabs(o.fix_alpha_value + 1.) <= 2.220446049250313e-16) o.fix_alpha = 0;   // (-1 is "not given" there)
  if (svd == "Empty") {
    if (ud == "Empty") die("--UDPath is required when --RefVCF is absent");
    if (mu == "Empty") die("--MeanPath is required when --RefVCF is absent");
    if (bed == "Empty") die("--BedPath is required when --RefVCF is absent");
  }
  if (pileup == "Empty") die("--BamFile or --PileupFile is required (--PileupFile here)");
  if (!known_af.empty()) o.known_af = known_af.c_str();
  if (!o.host_eval) fq_runtime_configure(0, 1);
  fq_popcon_t *p = nullptr;
  if (fq_popcon_create(svd == "Empty" ? nullptr : svd.c_str(), ud.c_str(), mu.c_str(), bed.c_str(), &o, &p)) die(fq_popcon_last_error(nullptr));
  auto fail = [&](const char *what) { const std::string m = std::string(what) + ": " + fq_popcon_last_error(p); fq_popcon_destroy(p); die(m); };
  if (fq_popcon_set_pileup_file(p, pileup.c_str())) fail("pileup");
  if (fq_popcon_run(p)) fail("pop+con");
  if (fq_popcon_write(p, out.c_str())) fail("output");
  fq_popcon_result_t r;
  fq_popcon_result(p, &r);
  fprintf(stderr, "NOTICE - FREEMIX %g, %lld likelihood evaluations over %d of %d markers (%s)\n", r.alpha < 0.5 ? r.alpha : 1 - r.alpha, (long long)r.n_eval, r.markers_used, r.n_marker,
          o.host_eval ? "host loop" : "device kernels");
  fq_popcon_destroy(p);
  fprintf(stderr, "NOTICE - Success!\n");
  return 0;
}

// `FASTQuick pop+con --RefVCF` (vb2Main.cpp:119-131: SVDcalculator::ProcessRefVCF): P.UD, P.mu, P.V and P.bed of a reference panel; P defaults to the VCF's path
static int svd_main(int argc, char **argv) {
  if (!fq_svd_create) die("svd: this build of the library has no SVD calculator");
  fq_svd_opts_t o;
  fq_svd_default_opts(&o);
  std::string vcf, list, sites, out, reader;
  for (int i = 2; i < argc; ++i) {
    const std::string f = argv[i];
    auto need = [&]() -> const char * { if (i + 1 >= argc) die("missing value for " + f); return argv[++i]; };
    if (f == "--RefVCF") vcf = need();
    else if (f == "--RefVCFList") list = need();
    else if (f == "--Sites") sites = need();
    else if (f == "--reader") reader = need();
    else if (f == "--chunk_bytes") o.chunk_bytes = atoll(need());
    else if (f == "--Output") out = need();
    else if (f == "--host_eval") o.host_eval = 1;
    else if (f == "--device") o.device = atoi(need());
    else die("unknown option " + f);
  }
  if (vcf.empty() && list.empty()) die("svd: --RefVCF is required (or --RefVCFList)");
  if (!vcf.empty() && !list.empty()) die("svd: --RefVCF and --RefVCFList exclude each other");
  // the reader: the serial one for a single VCF unless --reader says otherwise; a list or --Sites is the chunked reader's
  const bool chunked_input = !list.empty() || !sites.empty();
  if (reader.empty()) o.reader = chunked_input ? (o.host_eval ? 2 : 1) : 0;
  else if (reader == "serial") o.reader = 0;
  else if (reader == "device") o.reader = 1;
  else if (reader == "host_loops") o.reader = 2;
  else die("svd: --reader is serial, device or host_loops");
  if (o.reader == 0 && chunked_input) die("svd: --reader serial reads one --RefVCF: --RefVCFList and --Sites need the device or host_loops reader");
  if (o.chunk_bytes < 0) die("svd: --chunk_bytes must be positive");
  if (o.reader != 0 && !fq_svd_read_panel) die("svd: this build of the library has no chunked reader");
  std::vector<std::string> files;
  if (!list.empty()) {
    if (out.empty()) die("svd: --RefVCFList needs --Output");
    std::ifstream lf(list);
    if (!lf) die("svd: cannot open " + list);
    for (std::string ln; std::getline(lf, ln);) {
      while (!ln.empty() && (ln.back() == '\r' || ln.back() == ' ' || ln.back() == '\t')) ln.pop_back();
      if (!ln.empty()) files.push_back(ln);
    }
    if (files.empty()) die("svd: " + list + " names no file");
  } else files.push_back(vcf);
  if (out.empty()) out = vcf;
  if (!o.host_eval || o.reader == 1) fq_runtime_configure(0, 1);
  fq_svd_t *p = nullptr;
  if (fq_svd_create(&o, &p)) die(fq_svd_last_error(nullptr));
  auto fail = [&](const char *what) { const std::string m = std::string(what) + ": " + fq_svd_last_error(p); fq_svd_destroy(p); die(m); };
  std::string read_note = "serial reader";
  if (o.reader == 0) { if (fq_svd_read_vcf(p, vcf.c_str())) fail("svd"); }
  else {
    std::vector<const char *> cp;
    for (const auto &x : files) cp.push_back(x.c_str());
    if (fq_svd_read_panel(p, cp.data(), (int32_t)cp.size(), sites.empty() ? nullptr : sites.c_str())) fail("svd");
    fq_svd_read_stats_t rs;
    fq_svd_read_stats(p, &rs);
    if (!sites.empty()) fprintf(stderr, "NOTICE - Sites: %lld given, %lld found in the panel, %lld not found\n", (long long)rs.sites, (long long)rs.sites_found, (long long)(rs.sites - rs.sites_found));
    char note[400];
    snprintf(note, sizeof note, "%s reader: %lld lines, %lld at sites, %lld on the host, %lld chunks, %lld members; inflate %.3f s, line index %.3f s, site %.3f s, genotype %.3f s, host %.3f s",
             o.reader == 1 ? "device" : "host_loops", (long long)rs.lines, (long long)rs.site_lines, (long long)rs.host_lines, (long long)rs.chunks, (long long)(rs.members + rs.members_host), rs.t_inflate,
             rs.t_lines, rs.t_site, rs.t_geno, rs.t_host);
    read_note = note;
  }
  fq_svd_result_t r;
  fq_svd_result(p, &r);
  fprintf(stderr, "NOTICE - Number of Markers:%d\nNOTICE - Number of Individuals:%d\n", r.n_marker, r.n_sample);
  if (fq_svd_run(p)) fail("svd");
  if (fq_svd_write(p, out.c_str())) fail("output");
  fq_svd_result(p, &r);
  fprintf(stderr, "NOTICE - sigma_0 %g, %d iterations, residual %.3g (%s); read %.3f s, Gram %.3f s, iteration %.3f s, projection %.3f s, write %.3f s; %s\n", r.sigma[0], r.iterations, r.residual,
          o.host_eval ? "host loops" : "device kernels", r.t_read, r.t_gram, r.t_iter, r.t_project, r.t_write, read_note.c_str());
  fq_svd_destroy(p);
  fprintf(stderr, "NOTICE - Success!\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return usage();
  const std::string cmd = argv[1];
  if (cmd == "pop+con") return popcon_main(argc, argv);
  if (cmd == "svd") return svd_main(argc, argv);
  if (cmd == "index") {
    std::string ref;
    int rollhash = 0;
    for (int i = 2; i < argc; ++i) {
      if (!strcmp(argv[i], "--ref") && i + 1 < argc) ref = argv[++i];
      else if (!strcmp(argv[i], "--rollhash")) rollhash = 1;
      else return usage();
    }
    if (ref.empty()) return usage();
    const int rc = fq_index_build(ref.c_str(), rollhash);
    if (rc) die("fq_index_build failed (" + std::to_string(rc) + ")");
    return 0;
  }
  if (cmd != "align") return usage();
  Run R;
  Args &A = R.A;
  fq_default_opts(&A.o);
  for (int i = 2; i < argc; ++i) {
    const std::string f = argv[i];
    auto need = [&](const char *) -> const char * { if (i + 1 >= argc) die("missing value for " + f); return argv[++i]; };
    if (f == "--fastq_1") A.fq1 = need("");
    else if (f == "--fastq_2") A.fq2 = need("");
    else if (f == "--out_prefix") A.out_prefix = need("");
    else if (f == "--index_prefix") A.index_prefix = need("");
    else if (f == "--sam_out") A.sam_out = true;
    else if (f == "--kmer_thresh") A.o.filter_thresh = atoi(need(""));
    else if (f == "--n") A.o.fnr = atof(need(""));
    else if (f == "--o") A.o.max_gapo = atoi(need(""));
    else if (f == "--e") A.opte = atoi(need(""));
    else if (f == "--i") A.o.indel_end_skip = atoi(need(""));
    else if (f == "--d") A.o.max_del_occ = atoi(need(""));
    else if (f == "--l") A.o.seed_len = atoi(need(""));
    else if (f == "--k") A.o.max_seed_diff = atoi(need(""));
    else if (f == "--m") A.o.max_entries = atoi(need(""));
    else if (f == "--t") { A.o.host_threads = atoi(need("")); if (A.o.host_threads > 0) A.pack_threads = A.o.host_threads; }   // accepted for command-line compatibility (see fastquick_amd.h)
    else if (f == "--R") A.o.max_top2 = atoi(need(""));
    else if (f == "--q") A.o.trim_qual = atoi(need(""));
    else if (f == "--N") { A.o.mode |= 0x10; A.o.max_top2 = 0x7fffffff; }
    else if (f == "--L") A.o.mode |= 4;
    else if (f == "--I") A.o.mode |= 0x200;   // BWA_MODE_IL13
    else if (f == "--max_isize") A.o.max_isize = atoi(need(""));
    else if (f == "--max_occ") A.o.max_occ = (uint32_t)atoi(need(""));
    else if (f == "--is_sw") A.o.is_sw = !A.o.is_sw;          // a bool flag on a default-1 int: it toggles (src/FASTQuick.cpp:278)
    else if (f == "--n_multi") A.o.n_multi = atoi(need(""));
    else if (f == "--N_multi") A.o.N_multi = atoi(need(""));
    else if (f == "--ap_prior") A.o.ap_prior = atof(need(""));
    else if (f == "--force_isize") A.o.force_isize = 1;
    else if (f == "--chunk_pairs") A.chunk_pairs = atoll(need(""));
    else if (f == "--read_len") A.read_len = atoi(need(""));
    else if (f == "--clean_names") A.clean_names = true;
    else if (f == "--strict_reference") A.strict = true;
    else if (f == "--host_reader") A.host_reader = true;
    else if (f == "--host_consumers") A.host_consumers = true;
    else if (f == "--sorted_bam") A.sorted_bam = true;
    else if (f == "--bam_deflate") {
      const std::string m = need("");
      if (m == "fixed") A.bam_deflate = FQ_DEFLATE_FIXED; else if (m == "dynamic") A.bam_deflate = FQ_DEFLATE_DYNAMIC; else die("--bam_deflate takes fixed or dynamic, not " + m);
    }
    else if (f == "--sort_mem") { A.sort_mem = atoll(need("")); if (A.sort_mem < 0) die("--sort_mem must not be negative"); }
    else if (f == "--batch_pairs") A.o.batch_pairs = atoi(need(""));   // READ_BUFFER_SIZE of the run to reproduce (default 262144)
    else if (f == "--device") A.device = atoi(need(""));
    else if (f == "--devices") A.devices = need("");
    else if (f == "--fq_list") A.fq_list = need("");
    else if (f == "--RG") A.rg = need("");
    else if (f == "--cal_dup") A.cal_dup = !A.cal_dup;        // (a bool flag on a default-1 field, like --is_sw)
    else if (f == "--frac_samp") A.frac = atof(need(""));
    else if (f == "--bam_in") A.bam_in = need("");
    else if (f == "--collate") A.collate = true;
    else if (f == "--bam_rg") A.bam_rg.push_back(need(""));
    else if (f == "--bam_oq") A.bam_oq = true;
    else if (f == "--popcon_svd") A.popcon_svd = need("");
    else if (f == "--popcon_within") A.popcon_within = true;
    else if (f == "--popcon_numpc") A.popcon_numpc = atoi(need(""));
    else if (f == "--collate_mem") { A.collate_mem = atoll(need("")); A.collate_mem_given = true; if (A.collate_mem < 0) die("--collate_mem must not be negative"); }
    else die("unknown option " + f);
  }
  if (A.o.fnr >= 1.0) { A.o.max_diff = (int)A.o.fnr; A.o.fnr = -1.0; }                  // src/FASTQuick.cpp:312-315
  if (A.opte > 0) { A.o.max_gape = A.opte; A.o.mode &= ~1; }                             // :316-319
  // The reference re-allocates a read slot when a read longer than read_len arrives (src/BwtMapper.cpp:536-546).  That read then fills the
  // whole slot, so with read_len >= 96 -- the reference's own value is 151 -- nothing an earlier read left can reach the 96-base window the
  // read filter looks at, and the re-allocation is invisible; a smaller --read_len would make it visible, and is refused.
  if (A.read_len < 96) die("--read_len must be at least 96 (the reference's is 151): below that its slot re-allocation (src/BwtMapper.cpp:536-546) would show in the read filter, and it is not modelled");
  if (A.sorted_bam && A.sam_out) die("--sorted_bam writes a BAM file: it cannot be combined with --sam_out (sorting the SAM text is not supported)");
  if (A.bam_deflate >= 0 && A.sam_out) die("--bam_deflate chooses how the BAM file is compressed: it cannot be combined with --sam_out");
  if (A.collate && A.bam_in.empty()) die("--collate finds the mates of a BAM file: it needs --bam_in");
  if (!A.bam_rg.empty() && A.bam_in.empty()) die("--bam_rg selects read groups of a BAM file: it needs --bam_in (--RG names the output's group)");
  if (A.bam_oq && A.bam_in.empty()) die("--bam_oq reads the OQ qualities of a BAM file: it needs --bam_in");
  if (A.collate_mem_given && !A.collate) die("--collate_mem bounds what --collate holds: it needs --collate");
  if (A.popcon_svd.empty() && (A.popcon_within || A.popcon_numpc != 4)) die("--popcon_within and --popcon_numpc shape the estimate of --popcon_svd: they need it");
  if (A.popcon_numpc > 4 || A.popcon_numpc < 1) die("--popcon_numpc takes 1 to 4, as pop+con's --NumPC");
  if (A.out_prefix == "Empty") die("--out_prefix is required");
  if (A.index_prefix == "Empty") die("--index_prefix is required");
  R.inputs = read_inputs(A, !A.bam_in.empty() && probe_bam_input(A));
  if (A.o.batch_pairs < 1) die("--batch_pairs must be positive");
  A.chunk_pairs = std::max<long long>(A.o.batch_pairs, A.chunk_pairs / A.o.batch_pairs * A.o.batch_pairs);   // whole reference batches per chunk

  mark("options read");
  fq_runtime_configure(20, 1);   // hardware queues for the contexts' streams, sleeping waits: before the first HIP call (fastquick_amd.h)
  read_index_params(R);
  const bool shard_one_pair = pick_devices(R);
  if (R.wk.size() == 1) run_one_device(R);
  else if (shard_one_pair) run_sharded_pair(R);
  else run_list_over_devices(R);
  return 0;
}
