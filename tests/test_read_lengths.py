"""Read lengths over the whole accepted range (FQ_LMIN 15 ... FQ_LMAX 500) against the oracle, and the limits themselves.

The reference sustains reads of at most 256 bases (its StatCollector writes behind tables of 256 cycles for a longer mapped read, DESIGN.md
section 7), so above that the oracle is the yardstick: tests/golden/long256 and tests/fuzz_oracle_vs_reference.py hold the oracle to the reference
up to 256 bases, and the oracle's code has no branch on the length behind that.

One checker (check_case), run by the CPU tier on the host-loop backend (tests/emu: the kernel bodies, one lane) and by the GPU tier on the HIP
library, where the launchers choose a DP kernel by the length: fq_stats_t::dp_launches tells which one ran, and the GPU tests assert it.
Compared as test_gpu_parity.py::test_gpu_matches_oracle_on_fresh_inputs compares: stage dumps, SAM text (formatted on both sides, api.Aligner.sam_text),
filter_probes and gap_occ_touches.  No case may pass empty: survivors always; DP tasks and a gapped CIGAR where a case names a DP path."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util  # noqa: F401
import oracle_binding as ob
from fastquick_amd import api, synth

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
DP = {"refine_wave": 0, "refine_lds": 1, "refine": 2, "sw_wave_lds": 3, "sw_wave_global": 4, "sw_thread": 5}      # FQ_DP_* of fastquick_amd.h
QC_FILES = ["InsertSizeTable", "DepthDist", "GCDist", "EmpRepDist", "EmpCycleDist", "RawInsertSizeDist", "SexChromInfo", "Pileup",
            "FASTQ.csv", "Sequence.csv", "Summary", "AdjustedInsertSizeDist", "vcf"]
UNIFORM = [96, 97, 127, 128, 129, 191, 192, 193, 249, 251, 255, 256, 257, 319, 320, 321, 336, 344, 352, 368, 383, 384, 385, 447, 448, 449, 499, 500]
RAGGED = [(15, 500), (15, 95), (96, 250), (251, 500)]
N_PAIRS = 400


class Side:
    """the library under test and, per session, one reference whose every marker has the long flank (a window of 2001 bases holds a fragment of
    two 500-base reads), its index, and the oracle's output per input (the oracle does not depend on the knobs of the side under test)"""

    def __init__(self, lib, gpu, tmp):
        self.lib, self.gpu, self.tmp = lib, gpu, str(tmp)
        self.ref = synth.make_reference(n_markers=20, n_long=20, seed=811)
        self.pre = os.path.join(self.tmp, "ref.FASTQuick.fa")
        self.ref.write_fasta(self.pre)
        api.build_index(self.pre, lib=lib)
        synth.write_qc_inputs(self.pre, self.ref)
        self.ix = api.Index(self.pre, device=0, lib=lib) if gpu else api.Index(self.pre, lib=lib)
        self.oracle = {}
        self.serial = 0

    def path(self, stem):
        self.serial += 1
        return os.path.join(self.tmp, "%s_%d" % (stem, self.serial))


@pytest.fixture(scope="module")
def emu_side(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "libfq_emu.so"])
    return Side(api.load_library(os.path.join(EMU_DIR, "libfq_emu.so")), False, tmp_path_factory.mktemp("len_emu"))


@pytest.fixture(scope="module")
def gpu_side(tmp_path_factory):
    return Side(api.load_library(), True, tmp_path_factory.mktemp("len_gpu"))


def uniform_reads(side, L, n=N_PAIRS, chimera_frac=0.08, **kw):
    """indels of 1 to 3 bases (refinement), chimeric mates (mate rescue), a fragment that fits the read length"""
    args = dict(read_len=L, on_target=0.9, seed=4000 + L, sub_rate=0.01, del_frac=0.06, ins_frac=0.05, indel_len_max=3, chimera_frac=chimera_frac,
                frag_mean=L + (250 if L >= 150 else 120), frag_sd=30 if L >= 150 else 20)
    args.update(kw)
    return synth.make_reads(side.ref, n, **args)


def ragged_reads(side, lo, hi, batch, se=False, n=N_PAIRS):
    """the recipe of tests/fuzz_parity.py --ragged: lengths drawn per read; rows carry the read slots' history (Q7), or zeroed tails for single-end"""
    rb = uniform_reads(side, hi, n=n, frag_mean=max(hi, 150) + 200)
    rb.lens[:] = np.random.default_rng(1000 * lo + hi).integers(lo, hi + 1, rb.lens.shape)
    if se:
        for e in range(2):
            for i in range(rb.seq.shape[1]):
                rb.seq[e, i, rb.lens[e, i]:] = 0
    else:
        ob.apply_slot_history(rb.seq, rb.lens, batch)
    return rb


def oracle_output(side, key, rb, batch, se, okw):
    if key not in side.oracle:
        st, sam = side.path("orc.stages"), side.path("orc.sam")
        oa = ob.OracleAligner(side.pre, ob.default_opts(**okw))
        if se:
            oa.align_se(list(rb.names), rb.seq[0], rb.qual[0], rb.lens[0], st, sam, batch=batch)
        else:
            oa.align(rb.names, rb.seq, rb.qual, rb.lens, st, sam, batch=batch)
        side.oracle[key] = (st, open(sam, "rb").read(), oa.counters())
        oa.close()
    return side.oracle[key]


GAPPED = re.compile(rb"^\d+M(\d+[MIDS])*\d+[ID]\d+M")


def check_case(side, key, rb, batch=N_PAIRS, tuning=None, packed=False, se=False, dp=False, want=(), okw=None):
    """The side's stage dumps, SAM text and work counters against the oracle's for the reads rb.  dp: the case is about a DP path (tasks and a
    gapped CIGAR must exist); want: the DP variants the HIP launchers must have chosen (GPU side).  Returns the stats."""
    okw = okw or {}
    st_want, sam_want, oc = oracle_output(side, key, rb, batch, se, okw)
    al = api.Aligner(side.ix, api.default_opts(side.lib, batch_pairs=batch, single_end=1 if se else 0, **okw), max_pairs=batch, debug=True, tuning=tuning or {})
    st, sam = side.path("got.stages"), side.path("got.sam")
    survivors = []
    orig_align, orig_packed = al.align, al.align_packed

    def counting(fn):
        def run(*a):
            res = fn(*a)
            survivors.append(res.n_survivors)
            return res
        return run
    al.align, al.align_packed = counting(orig_align), counting(orig_packed)
    if se:
        api.align_stream(al, list(rb.names), rb.seq[:1], rb.qual[:1], rb.lens[:1], batch, st, sam)
    else:
        api.align_stream(al, rb.names, rb.seq, rb.qual, rb.lens, batch, st, sam, packed=packed)
    gs = al.stats()
    al.close()
    diffs = [d for d in ob.diff_stage_files(st_want, st)]
    assert not diffs, "\n".join(diffs)
    text = open(sam, "rb").read()
    assert text == sam_want, "SAM text differs from the oracle's"
    assert gs["filter_probes"] == oc["filter_probes"] and gs["gap_occ_touches"] == oc["occ_gap_touches"]
    assert sum(survivors) > 0, "nothing survived the filter: the input is the wrong one"
    if dp:
        assert gs["sw_tasks"] > 0 and gs["refine_tasks"] > 0, "no DP task: the input is the wrong one"
        cigars = [ln.split(b"\t")[5] for ln in text.split(b"\n") if ln and not ln.startswith(b"@")]
        assert any(GAPPED.match(c) for c in cigars), "no record with a gapped CIGAR"
    if side.gpu:
        for v in want:
            assert gs["dp_launches"][DP[v]] > 0, "%s was not launched (dp_launches %s)" % (v, gs["dp_launches"])
    else:
        assert not any(gs["dp_launches"]), "the host-loop backend has one loop per DP"
    return gs


# ---- uniform lengths -----------------------------------------------------------------------------------------------------------
def check_uniform(side, L):
    return check_case(side, ("uniform", L), uniform_reads(side, L), dp=True)


@pytest.mark.parametrize("L", UNIFORM)
def test_uniform_length_on_the_host_loop_backend(L, emu_side):
    check_uniform(emu_side, L)


@pytest.mark.gpu
def test_uniform_lengths_on_the_gpu(gpu_side):
    """every length of the sweep; from the launch counters: the refinement DP goes from k_refine_wave (row arrays and trace in 64 KiB of LDS) to
    k_refine (global scratch) somewhere in 320 ... 368 bases, and both ran.  The lengths on either side of the hand-over are printed."""
    ran = {}
    for L in UNIFORM:
        gs = check_uniform(gpu_side, L)
        d = gs["dp_launches"]
        assert d[DP["refine_wave"]] + d[DP["refine"]] > 0 and d[DP["refine_lds"]] == 0, "no production shape selects k_refine_lds (%d bases: %s)" % (L, d)
        assert d[DP["sw_wave_lds"]] + d[DP["sw_wave_global"]] > 0 and d[DP["sw_thread"]] == 0, "%d bases: %s" % (L, d)
        ran[L] = d
        print("L %3d dp_launches %s sw_tasks %d refine_tasks %d" % (L, d, gs["sw_tasks"], gs["refine_tasks"]))
    span = [L for L in UNIFORM if 320 <= L <= 368]
    wave = [L for L in span if ran[L][DP["refine_wave"]]]
    lane = [L for L in span if ran[L][DP["refine"]]]
    print("k_refine_wave at %s, k_refine at %s" % (wave, lane))
    assert wave and lane, "both refinement kernels were to run between 320 and 368 bases"
    assert max(wave) < min(lane), "the hand-over is one length, not a mixture"
    assert all(ran[L][DP["refine_wave"]] and not ran[L][DP["refine"]] for L in UNIFORM if L < 320)
    assert all(ran[L][DP["refine"]] and not ran[L][DP["refine_wave"]] for L in UNIFORM if L > 368)
    # mate rescue at 500 bases: the trace matrix of a window that holds the query is (RL + 1)(QL + 1) >= 501 x 501 bytes, beyond the kernel's
    # 150 KiB of LDS whatever the number of tasks, so the trace lies in global scratch (both placements at 150 bases: test_few_and_many_rescue_tasks_*)
    assert ran[500][DP["sw_wave_global"]] and not ran[500][DP["sw_wave_lds"]]
    # ... and in LDS around 250 bases, where the query is 4 stripes of 64 rows with a partial last one (249, 251, 255), a full one (256) or a fifth
    # stripe of one row (257): some 60 tasks, windows of about 700 bases, a trace of about 180 KB only from 300-base queries on
    for L in (249, 251, 255, 256, 257):
        assert ran[L][DP["sw_wave_lds"]] and not ran[L][DP["sw_wave_global"]], "%d bases: %s" % (L, ran[L])


# ---- ragged batches ------------------------------------------------------------------------------------------------------------
BOUNDARIES = {"ascii": dict(), "packed": dict(packed=True, tuning={"packed_bulk_min": 1 << 30}), "packed_bulk": dict(packed=True, tuning={"packed_bulk_min": 0}), "single_end": dict(se=True)}


def check_ragged(side, lo, hi, boundary):
    kw = BOUNDARIES[boundary]
    se = bool(kw.get("se"))
    batch = 200      # two batches: the slots' history crosses one
    check_case(side, ("ragged", lo, hi, se), ragged_reads(side, lo, hi, batch, se=se), batch=batch, **kw)


@pytest.mark.parametrize("boundary", list(BOUNDARIES))
@pytest.mark.parametrize("lo,hi", RAGGED)
def test_ragged_batch_on_the_host_loop_backend(lo, hi, boundary, emu_side):
    check_ragged(emu_side, lo, hi, boundary)


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", list(BOUNDARIES))
@pytest.mark.parametrize("lo,hi", RAGGED)
def test_ragged_batch_on_the_gpu(lo, hi, boundary, gpu_side):
    check_ragged(gpu_side, lo, hi, boundary)


# ---- knobs: the paths no production shape (or only some) selects -----------------------------------------------------------------
def knob_inputs(side):
    return [("u150", ("uniform", 150), lambda: uniform_reads(side, 150), 150), ("u250", ("uniform", 250), lambda: uniform_reads(side, 250), 250),
            ("u500", ("uniform", 500), lambda: uniform_reads(side, 500), 500), ("r251_500", ("ragged", 251, 500, False), lambda: ragged_reads(side, 251, 500, 200), 500)]


def check_knobs(side, which):
    for tag, key, make, longest in knob_inputs(side):
        if tag != which:
            continue
        rb = make()
        batch = 200 if tag.startswith("r") else N_PAIRS
        # the lane-per-task refinement kernels: rows in LDS while 3 x (RL + 1) x 64 x 4 bytes fit 150 KiB (RL <= 199), global scratch above.  RL is the
        # longest reference stretch of a task, the read and its band: 150 bases stay below 199, 250 and more lie above
        gs = check_case(side, key, rb, batch=batch, tuning={"refine_lanes": 1}, dp=True, want=["refine_lds" if longest <= 150 else "refine"])
        if side.gpu:      # one lane kernel for the whole batch, never a mixture
            other = "refine" if longest <= 150 else "refine_lds"
            assert gs["dp_launches"][DP["refine_wave"]] == 0 and gs["dp_launches"][DP[other]] == 0, gs["dp_launches"]
        # every mate-rescue window above sw_wave_max goes to the task-per-lane kernel: 14 is below any window (a window holds a read of FQ_LMIN at least)
        gs = check_case(side, key, rb, batch=batch, tuning={"sw_wave_max": 14}, dp=True, want=["sw_thread"])
        if side.gpu:
            assert gs["dp_launches"][DP["sw_wave_lds"]] + gs["dp_launches"][DP["sw_wave_global"]] == 0
        check_case(side, key, rb, batch=batch, tuning={"sw_serial_reverse": 1}, dp=True)
        gs = check_case(side, key, rb, batch=batch, tuning={"gap_long_pops": 1, "gap_long_always": 1}, dp=True)
        assert gs["tier_retries"] > 0, "the wavefront-per-read search kernel was to take every read"
        check_case(side, key, rb, batch=batch, tuning={"gap_nogap_min": 0}, dp=True)
        check_case(side, key, rb, batch=batch, tuning={"gap_nogap_min": 0, "gap_generic_opts": 1}, dp=True)


KNOB_INPUTS = ["u150", "u250", "u500", "r251_500"]


@pytest.mark.parametrize("which", KNOB_INPUTS)
def test_knob_runs_on_the_host_loop_backend(which, emu_side):
    check_knobs(emu_side, which)


@pytest.mark.gpu
@pytest.mark.parametrize("which", KNOB_INPUTS)
def test_knob_runs_on_the_gpu(which, gpu_side):
    check_knobs(gpu_side, which)


def check_many_rescue_tasks(side):
    """the trace matrix of k_sw_wave lies in LDS only for launches of at most 256 tasks: 150-base reads with few chimeric mates (the sweep's
    input) against 3,000 pairs of which a third are chimeric, in one call"""
    few = check_case(side, ("uniform", 150), uniform_reads(side, 150), dp=True, want=["sw_wave_lds"])
    assert 0 < few["sw_tasks"] <= 256
    many = check_case(side, ("many", 150), uniform_reads(side, 150, n=3000, chimera_frac=0.35), batch=3000, dp=True, want=["sw_wave_global"])
    assert many["sw_tasks"] > 256
    if side.gpu:
        assert few["dp_launches"][DP["sw_wave_global"]] == 0 and many["dp_launches"][DP["sw_wave_lds"]] == 0


def test_few_and_many_rescue_tasks_on_the_host_loop_backend(emu_side):
    check_many_rescue_tasks(emu_side)


@pytest.mark.gpu
def test_few_and_many_rescue_tasks_on_the_gpu(gpu_side):
    check_many_rescue_tasks(gpu_side)


# ---- consumers: the device's BAM records and QC sums against the host's on the same results ------------------------------------------
def bam_bytes(path):
    return gzip.open(path, "rb").read()


def check_consumers(side, which):
    if which == "r251_500":
        rb, batch, key = ragged_reads(side, 251, 500, 200), 200, ("ragged", 251, 500, False)
    else:
        rb, batch, key = uniform_reads(side, which), N_PAIRS, ("uniform", which)
    fq1, fq2 = rb.write_fastq(side.path("cons"))
    fai = side.path("genome.fai")
    with open(fai, "w") as fh:
        for chrom in sorted({nm.split(":")[0] for nm in side.ref.names}):
            fh.write("%s\t%d\t%d\t60\t61\n" % (chrom, len(side.ref.genome), len(chrom) + 2))
    read_len = int(rb.lens.max()) + 1
    out = {}
    for on_device in (False, True):
        al = api.Aligner(side.ix, api.default_opts(side.lib, batch_pairs=batch), max_pairs=batch)
        stem = side.path("dev" if on_device else "host")
        bam = api.BamWriter(side.ix, fai, stem + ".bam")
        qc = api.QC(side.ix, side.pre, stem + ".qc", genome_size=len(side.ref.genome), read_len=read_len)
        if on_device:
            bam.attach(al)
            qc.attach(al)
        qc.begin_file(fq1, fq2)
        mapped = api.align_stream(al, rb.names, rb.seq, rb.qual, rb.lens, batch, None, None, qc=qc, bam=bam)
        assert mapped > 0
        qc.end_file()
        qc.write()
        qc.close(); bam.close(); al.close()
        out[on_device] = stem
    host, dev = bam_bytes(out[False] + ".bam"), bam_bytes(out[True] + ".bam")
    assert len(host) > 1000 and dev == host, "BAM records formatted on the device differ from the host writer's"
    for f in QC_FILES:
        a, b = (open(out[d] + ".qc." + f, "rb").read() for d in (False, True))
        if f == "vcf":
            a, b = (b"\n".join(ln for ln in t.split(b"\n") if not ln.startswith(b"##fileDate=")) for t in (a, b))
        assert a == b, "QC file %s of the device consumer differs from the host consumer's" % f
    # ... and the results under them are the oracle's
    check_case(side, key, rb, batch=batch)


CONSUMER_INPUTS = [251, 499, 500, "r251_500"]


@pytest.mark.parametrize("which", CONSUMER_INPUTS)
def test_consumers_on_the_host_loop_backend(which, emu_side):
    check_consumers(emu_side, which)


@pytest.mark.gpu
@pytest.mark.parametrize("which", CONSUMER_INPUTS)
def test_consumers_on_the_gpu(which, gpu_side):
    check_consumers(gpu_side, which)


# ---- the limits ----------------------------------------------------------------------------------------------------------------
def check_limits(side, bad_len):
    """a read of 501 (14) bases is refused with FQ_ELIMIT at every boundary; the next valid batch on the same context gives the oracle's output"""
    good = uniform_reads(side, 500 if bad_len > 500 else 96, n=64)
    key = ("limit_good", bad_len)
    st_want, sam_want, _ = oracle_output(side, key, good, 64, False, {})
    body = sam_want[len(side.ix.sam_header()):]
    width = max(bad_len, good.seq.shape[2])
    seq = np.full((2, 64, width), ord("A"), dtype=np.uint8); qual = np.full((2, 64, width), ord("F"), dtype=np.uint8)
    seq[:, :, :good.seq.shape[2]] = good.seq; qual[:, :, :good.qual.shape[2]] = good.qual
    ragged_lens = good.lens.copy(); ragged_lens[1, 7] = bad_len
    uniform_lens = np.full((2, 64), bad_len, dtype=np.int32)
    for boundary, lens in (("ascii", ragged_lens), ("packed", ragged_lens), ("packed", uniform_lens)):
        al = api.Aligner(side.ix, api.default_opts(side.lib, batch_pairs=64), max_pairs=64)
        with pytest.raises(api.FastquickError, match=r"-5 \(read length outside \[15,500\]\)"):
            if boundary == "ascii":
                al.align(seq, qual, lens, good.names)
            else:
                bad = api.HostPacked(seq, qual, lens, good.names, lib=side.lib)
                try:
                    al.align_packed(bad)
                finally:
                    al._keep_packed = None
                    bad.free()
        if boundary == "ascii":
            res = al.align(good.seq, good.qual, good.lens, good.names)
        else:
            hp = api.HostPacked(good.seq, good.qual, good.lens, good.names, lib=side.lib)
            res = al.align_packed(hp)
        assert res.n_survivors > 0
        assert al.sam_text() == body, "the batch after a refused one (%s) differs from the oracle's" % boundary
        if boundary != "ascii":
            al._keep_packed = None
            hp.free()
        al.close()


@pytest.mark.parametrize("bad_len", [501, 14])
def test_limits_on_the_host_loop_backend(bad_len, emu_side):
    check_limits(emu_side, bad_len)


@pytest.mark.gpu
@pytest.mark.parametrize("bad_len", [501, 14])
def test_limits_on_the_gpu(bad_len, gpu_side):
    check_limits(gpu_side, bad_len)


def fastq_text(rb, end, lo=0, hi=None):
    hi = rb.seq.shape[1] if hi is None else hi
    return b"".join(b"@" + bytes(rb.names[i]) + b"\n" + bytes(rb.seq[end, i, :rb.lens[end, i]]) + b"\n+\n" + bytes(rb.qual[end, i, :rb.lens[end, i]]) + b"\n" for i in range(lo, hi))


def write_pair(side, rb, stem, bgzf):
    paths = []
    for e in range(2):
        p = side.path(stem) + "_%d.fq%s" % (e + 1, ".gz" if bgzf else "")
        with open(p, "wb") as fh:
            fh.write(synth.bgzf_compress(fastq_text(rb, e), threads=2, level=6, member=4000) if bgzf else fastq_text(rb, e))
        paths.append(p)
    return paths


def with_bad_read(good, at, bad_len):
    """the reads of `good` in rows wide enough for bad_len, read 2 of pair `at` with bad_len bases"""
    n, width = good.seq.shape[1], max(bad_len, good.seq.shape[2])
    seq = np.full((2, n, width), ord("A"), dtype=np.uint8); qual = np.full((2, n, width), ord("F"), dtype=np.uint8)
    seq[:, :, :good.seq.shape[2]] = good.seq; qual[:, :, :good.qual.shape[2]] = good.qual
    lens = good.lens.copy()
    lens[1, at] = bad_len
    return synth.ReadBatch(seq, qual, lens, list(good.names))


def check_text_batch_limits(side, bad_len, uniform):
    """the text batch of the device front end (fq_align_text): a batch with a read of 501 (14) bases -- one read of it, or every read -- is refused
    with FQ_ELIMIT; the next batch of the same front end on the same context gives the oracle's output"""
    B = 64
    base = 500 if bad_len > 500 else 96
    good = uniform_reads(side, base, n=2 * B)
    rb = with_bad_read(good, 7, bad_len)
    if uniform:
        rb.lens[:, :B] = bad_len
    second = synth.ReadBatch(good.seq[:, B:], good.qual[:, B:], good.lens[:, B:], good.names[B:])
    _, sam_want, _ = oracle_output(side, ("text_limit", base), second, B, False, {})
    fq = write_pair(side, rb, "textlimit", bgzf=True)
    kw = dict(device=0) if side.gpu else {}
    fe = api.DeviceFrontEnd(fq[0], fq[1], batch_pairs=B, chunk_pairs=B, slot_mode=1, max_read_len=512, lib=side.lib, **kw)
    al = api.Aligner(side.ix, api.default_opts(side.lib, batch_pairs=B), max_pairs=B)
    n, b = fe.next()
    assert n == B
    with pytest.raises(api.FastquickError, match=r"-5 \(read length outside \[15,500\]\)"):
        al.align_text(b)
    fe.release(b)
    n, b = fe.next()
    assert n == B
    res = al.align_text(b)
    assert res.n_survivors > 0
    assert side.ix.sam_header() + al.sam_text() == sam_want, "the text batch after a refused one differs from the oracle's"
    fe.release(b)
    n, b = fe.next()
    assert n == 0 and fe.stats()["refused"] == 0
    fe.close(); al.close()


TEXT_LIMITS = [(501, False), (501, True), (14, False)]


@pytest.mark.parametrize("bad_len,uniform", TEXT_LIMITS)
def test_text_batch_limits_on_the_host_loop_backend(bad_len, uniform, emu_side):
    check_text_batch_limits(emu_side, bad_len, uniform)


@pytest.mark.gpu
@pytest.mark.parametrize("bad_len,uniform", TEXT_LIMITS)
def test_text_batch_limits_on_the_gpu(bad_len, uniform, gpu_side):
    check_text_batch_limits(gpu_side, bad_len, uniform)


# ---- the command line --------------------------------------------------------------------------------------------------------------
GPU_CLI = os.path.join(os.path.dirname(HERE), "fastquick_amd", "bin", "FASTQuick_amd")


def run_cli(exe, prefix, fq, batch, *extra):
    cmd = [exe, "align", "--index_prefix", prefix[:-len(".FASTQuick.fa")], "--fastq_1", fq[0], "--fastq_2", fq[1], "--out_prefix", fq[0] + ".out",
           "--sam_out", "--batch_pairs", str(batch), "--chunk_pairs", str(batch)] + [str(x) for x in extra]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def check_cli_long_reads(side, exe, golden):
    """--sam_out through the device front end (BGZF files) and through --host_reader, with --read_len = length + 1 and without it (the row stride
    then comes from the first records): the reference's text for the 256-base golden, the oracle's for 500-base reads"""
    g = golden
    rb = uniform_reads(side, 500, n=192)
    _, sam500, _ = oracle_output(side, ("cli", 500), rb, 64, False, {})
    gz = {"fq1": None, "fq2": None}
    for k in gz:
        gz[k] = side.path("long256") + ".fq.gz"
        with open(gz[k], "wb") as fh:
            fh.write(synth.bgzf_compress(open(g[k], "rb").read(), threads=2, level=6, member=4000))
    inputs = [("long256", g["prefix"], {"device": [gz["fq1"], gz["fq2"]], "host": [g["fq1"], g["fq2"]]}, g["batch"], open(g["sam"], "rb").read(), 257),
              ("u500", side.pre, {"device": write_pair(side, rb, "cli500", True), "host": write_pair(side, rb, "cli500", False)}, 64, sam500, 501)]
    for tag, prefix, files, batch, want, read_len in inputs:
        for mode in ("device", "host"):
            for extra in (["--read_len", read_len], []):
                run = run_cli(exe, prefix, files[mode], batch, *(extra + (["--host_reader"] if mode == "host" else [])))
                assert run.returncode == 0, run.stderr.decode(errors="replace")[-2000:]
                assert (b"front end on the device" in run.stderr) == (mode == "device"), (tag, mode)
                assert run.stdout == want, "%s through the %s reader, %s: SAM text differs" % (tag, mode, extra or "stride from the first records")


def check_cli_limit_in_the_third_chunk(side, exe):
    """a file whose third chunk holds a 501-base read: the records of the two chunks before it are printed, the run fails and names the limit"""
    B = 64
    good = uniform_reads(side, 500, n=3 * B)
    rb = with_bad_read(good, 2 * B + 5, 501)
    first = synth.ReadBatch(good.seq[:, :2 * B], good.qual[:, :2 * B], good.lens[:, :2 * B], good.names[:2 * B])
    _, want, _ = oracle_output(side, ("cli_third", 500), first, B, False, {})
    for mode in ("device", "host"):
        fq = write_pair(side, rb, "third", bgzf=(mode == "device"))
        run = run_cli(exe, side.pre, fq, B, *(["--host_reader"] if mode == "host" else []))
        assert run.returncode == 1, (mode, run.returncode, run.stderr.decode(errors="replace")[-1000:])
        assert run.stdout == want, "%s reader: the records of the chunks before the refused one differ from the oracle's (%d bytes vs %d)" % (mode, len(run.stdout), len(want))
        assert b"read length outside [15,500]" in run.stderr, run.stderr.decode(errors="replace")[-1000:]


def test_cli_long_reads_on_the_host_loop_backend(emu_side, emu_cli, golden_cases):
    check_cli_long_reads(emu_side, emu_cli, golden_cases["long256"])


def test_cli_limit_in_the_third_chunk_on_the_host_loop_backend(emu_side, emu_cli):
    check_cli_limit_in_the_third_chunk(emu_side, emu_cli)


@pytest.mark.gpu
def test_cli_long_reads_on_the_gpu(gpu_side, golden_cases):
    check_cli_long_reads(gpu_side, GPU_CLI, golden_cases["long256"])


@pytest.mark.gpu
def test_cli_limit_in_the_third_chunk_on_the_gpu(gpu_side):
    check_cli_limit_in_the_third_chunk(gpu_side, GPU_CLI)
