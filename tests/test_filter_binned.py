"""The binned form of the packed / text filter (tuning key filter_binned_min; fq_kernels.h "the same filter, binned"): count, bin by 2 MiB
region, probe, verdict.  Every case runs with filter_binned_min = 0 against the oracle -- stage dumps, SAM text, the reference's probe count --
through the HIP library (marked gpu) and, unmarked, through the host-loop backend, whose launcher runs the same phases as loops over the same routines
(tests/emu/fq_emu_binned.cpp: libfq_emu_binned.so, the CPU tier's host-loop library with that one launcher in front).  tests/emu/filter_binned_check.cpp
runs those loops once more as a program of its own under the address and undefined-behaviour sanitizers."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
from fastquick_amd import api, synth

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
BINNED = {"filter_binned_min": 0, "md_mask_min": 0}


class Side:
    def __init__(self, lib, gpu):
        self.lib, self.gpu = lib, gpu

    def index(self, pre):
        return api.Index(pre, device=0) if self.gpu else api.Index(pre, lib=self.lib)


@pytest.fixture(scope="module")
def gpu_side():
    return Side(api.load_library(), True)      # fastquick_amd/libfastquick_amd.so -- raises if missing: no fallback


@pytest.fixture(scope="module")
def emu_side():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "-f", "Makefile.binned"])
    return Side(api.load_library(os.path.join(EMU_DIR, "libfq_emu_binned.so")), False)


def plant_runs(genome, pos, flank, rng):
    """runs of 40 A and of 40 T in the flanks of every third marker: the 32-mers of all A and of all T (keys 0 and 2^32 - 1 of every table) are in the bitmaps"""
    for k in range(0, len(pos), 3):
        p, f = int(pos[k]), int(flank[k])
        genome[p - 1 - f + 20:p - 1 - f + 60] = 0
        genome[p + f - 70:p + f - 30] = 3


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """two small references, indexed once for both sides: a plain one, and one whose flanks hold runs of 40 A and 40 T"""
    out = {}
    for tag, kw in (("plain", dict(n_markers=24, n_long=2, seed=77, repeat_every=4)), ("runs", dict(n_markers=12, n_long=2, seed=79, patch=plant_runs))):
        ref = synth.make_reference(**kw)
        pre = str(tmp_path_factory.mktemp("binned_" + tag) / "ref.FASTQuick.fa")
        ref.write_fasta(pre)
        api.build_index(pre)
        out[tag] = (ref, pre)
    return out


_oracle = {}


def oracle_output(key, pre, rb, batch, se, okw, tmp):
    """stage dump, SAM text and counters of the oracle for a case: computed once, shared by the two sides, never changed"""
    if key not in _oracle:
        st, sam = os.path.join(tmp, "orc.stages"), os.path.join(tmp, "orc.sam")
        oa = ob.OracleAligner(pre, ob.default_opts(**okw))
        if se:
            oa.align_se(list(rb.names), rb.seq[0], rb.qual[0], rb.lens[0], st, sam, batch=batch)
        else:
            oa.align(rb.names, rb.seq, rb.qual, rb.lens, st, sam, batch=batch)
        _oracle[key] = (open(st, "rb").read(), open(sam, "rb").read(), oa.counters())
        oa.close()
    return _oracle[key]


def run_side(side, pre, rb, batch, se, okw, tuning, tmp, tag):
    ix = side.index(pre)
    al = api.Aligner(ix, api.default_opts(side.lib, batch_pairs=batch, single_end=1 if se else 0, **okw), max_pairs=max(16, batch), debug=True, tuning=tuning)
    st, sam = os.path.join(tmp, tag + ".stages"), os.path.join(tmp, tag + ".sam")
    if se:
        api.align_stream(al, list(rb.names), rb.seq[:1], rb.qual[:1], rb.lens[:1], batch, st, sam, packed=True)
    else:
        api.align_stream(al, rb.names, rb.seq, rb.qual, rb.lens, batch, st, sam, packed=True)
    gs = al.stats()
    al.close(); ix.close()
    return st, open(sam, "rb").read(), gs


def check(side, key, pre, rb, tmp_path, batch=None, se=False, okw=None, tuning=None):
    okw, tmp = okw or {}, str(tmp_path)
    batch = batch or rb.seq.shape[1]
    st_want, sam_want, oc = oracle_output(key, pre, rb, batch, se, okw, tmp)
    want = os.path.join(tmp, "want.stages")
    with open(want, "wb") as fh:
        fh.write(st_want)
    st, sam, gs = run_side(side, pre, rb, batch, se, okw, dict(BINNED, **(tuning or {})), tmp, "got")
    diffs = [d for d in ob.diff_stage_files(want, st)]
    assert not diffs, "\n".join(diffs)
    assert sam == sam_want, "SAM text differs from the oracle's"
    assert gs["filter_probes"] == oc["filter_probes"]
    n_reads = rb.seq.shape[1] * (1 if se else 2)
    assert gs["filter_binned_reads"] == n_reads > 0, "the binned form did not filter every read"
    assert gs["filter_bin_spill"] == 0
    return gs


# ---- the cases: (key, reference, reads, keywords of check) ------------------------------------------------------------------------------
def sized(refs, n, on):
    ref, pre = refs["plain"]
    return pre, synth.make_reads(ref, n, on_target=on, seed=500 + n, sub_rate=0.01, del_frac=0.04, ins_frac=0.03)


def case_size(refs, n, on):
    """1 .. 4,099 pairs: partial wavefronts, partial tiles of the bin kernel, far more buckets than probes; both verdicts, or only `filtered`"""
    pre, rb = sized(refs, n, on)
    return pre, rb, {}


def case_thresh(refs, th):
    """filter_thresh 1, 2: all 18 probes are binned; 3, 5: the last two fetched by the verdict; 19: nothing can pass"""
    pre, rb = sized(refs, 257, 0.5)
    return pre, rb, dict(okw=dict(filter_thresh=th))


def case_bulk(refs, bulk):
    pre, rb = sized(refs, 4099, 0.5)
    return pre, rb, dict(tuning={"packed_bulk_min": bulk}, batch=1500)      # (three calls on one context: the masks and counts left zero by the one before)


def case_single_end(refs):
    pre, rb = sized(refs, 257, 0.5)
    return pre, rb, dict(se=True)


def case_ragged(refs):
    """ragged lengths and trimming: len, qual_last, sub_max, sub_whole and the length counters come from the verdict kernel"""
    ref, pre = refs["plain"]
    rb = synth.make_reads(ref, 300, read_len=120, on_target=0.6, seed=611, qual_decay=True, sub_rate=0.01, frag_mean=300)
    rb.lens[:] = np.random.default_rng(612).integers(70, 121, rb.lens.shape)
    ob.apply_slot_history(rb.seq, rb.lens, 300)
    return pre, rb, dict(okw=dict(trim_qual=15))


def case_identical(refs):
    """4,096 copies of one pair: every probe of the launch in the same 16 buckets"""
    ref, pre = refs["runs"]
    one = synth.make_reads(ref, 1, on_target=1.0, seed=620)
    n = 4096
    rb = synth.ReadBatch(np.repeat(one.seq, n, axis=1), np.repeat(one.qual, n, axis=1), np.repeat(one.lens, n, axis=1), [b"i%09d" % i for i in range(n)])
    return pre, rb, {}


def case_homopolymer(refs, base):
    """the first 96 bases all A (every key 0: bucket 0x00, offset 0) or all T (every key 2^32 - 1: bucket 0xff, offset 2^24 - 1); the reference holds both runs"""
    ref, pre = refs["runs"]
    rb = synth.make_reads(ref, 4096, on_target=0.0, seed=630 + ord(base))
    rb.seq[:, :, :96] = ord(base)
    return pre, rb, {}


CASES = {}
for _n in (1, 63, 64, 65, 257, 4099):
    for _on, _mix in ((0.5, "half"), (0.0, "off")):
        CASES["size%d_%s" % (_n, _mix)] = (case_size, (_n, _on))
for _th in (1, 2, 3, 5, 19):
    CASES["thresh%d" % _th] = (case_thresh, (_th,))
CASES["bulk_all"] = (case_bulk, (0,))
CASES["bulk_never"] = (case_bulk, (1 << 30,))
CASES["single_end"] = (case_single_end, ())
CASES["ragged_trim15"] = (case_ragged, ())
CASES["identical"] = (case_identical, ())
CASES["poly_a"] = (case_homopolymer, ("A",))
CASES["poly_t"] = (case_homopolymer, ("T",))


def run_case(side, refs, tmp_path, key):
    fn, args = CASES[key]
    pre, rb, kw = fn(refs, *args)
    gs = check(side, key, pre, rb, tmp_path, **kw)
    if key in ("poly_a", "poly_t"):
        assert gs["reads_searched"] == 2 * 4096, "the planted runs must make every homopolymer head pass the filter"


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(CASES))
def test_binned_filter_matches_oracle_gpu(key, gpu_side, refs, tmp_path):
    run_case(gpu_side, refs, tmp_path, key)


@pytest.mark.parametrize("key", list(CASES))
def test_binned_filter_matches_oracle_host_loops(key, emu_side, refs, tmp_path):
    run_case(emu_side, refs, tmp_path, key)


def test_binned_routines_as_host_loops_equal_the_direct_statement(tmp_path):
    """count and offsets, bin, probe, verdict as loops over fq_kernels.h's routines: filtered[], sub_max, sub_whole and the counters of every case
    equal fq_prep_packed_thread's (sizes 1 .. 4,099, thresholds 1, 2, 3, 5, 19, ragged lengths with trimming, keys 0 and 2^32 - 1, one read repeated)"""
    root = os.path.dirname(EMU_DIR)
    exe = str(tmp_path / "filter_binned_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unused-function",
                           "-Wno-unused-variable", "-Wno-unknown-pragmas", "-I" + EMU_DIR, "-I" + os.path.join(root, "..", "fastquick_amd", "csrc"), "-I" + os.path.join(root, "..", "include"),
                           "-o", exe, os.path.join(EMU_DIR, "filter_binned_check.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), out.stdout[-2000:]


# ---- the two forms agree -----------------------------------------------------------------------------------------------------------------
def forms_agree(side, refs, tmp_path):
    pre, rb = sized(refs, 4099, 0.5)
    got = {}
    for tag, v in (("binned", 0), ("direct", 1 << 30)):
        st, sam, gs = run_side(side, pre, rb, 1500, False, {}, {"filter_binned_min": v, "md_mask_min": 0}, str(tmp_path), tag)
        got[tag] = (st, sam, gs)
    assert filecmp.cmp(got["binned"][0], got["direct"][0], shallow=False), "stage dumps of the two forms differ"
    assert got["binned"][1] == got["direct"][1]
    assert got["binned"][2]["filter_probes"] == got["direct"][2]["filter_probes"] > 0
    assert got["binned"][2]["filter_binned_reads"] == 2 * 4099 and got["direct"][2]["filter_binned_reads"] == 0


@pytest.mark.gpu
def test_the_two_forms_agree_gpu(gpu_side, refs, tmp_path):
    forms_agree(gpu_side, refs, tmp_path)


def test_the_two_forms_agree_host_loops(emu_side, refs, tmp_path):
    forms_agree(emu_side, refs, tmp_path)


# ---- a text batch of the device front end goes through the same seam ---------------------------------------------------------------------
def text_batch(side, refs, tmp_path):
    ref, pre = refs["plain"]
    rb = synth.make_reads(ref, 600, on_target=0.5, seed=640, sub_rate=0.01)
    _, sam_want, oc = oracle_output("text", pre, rb, 300, False, {}, str(tmp_path))
    fq = []
    for e in range(2):
        text = b"".join(b"@" + bytes(rb.names[i]) + b"\n" + bytes(rb.seq[e, i, :rb.lens[e, i]]) + b"\n+\n" + bytes(rb.qual[e, i, :rb.lens[e, i]]) + b"\n" for i in range(len(rb.names)))
        fq.append(str(tmp_path / ("reads_%d.fq.gz" % (e + 1))))
        with open(fq[e], "wb") as fh:
            fh.write(synth.bgzf_compress(text, threads=2, level=6, member=4000))
    ix = side.index(pre)
    fe = api.DeviceFrontEnd(fq[0], fq[1], batch_pairs=300, chunk_pairs=300, slot_mode=1, max_read_len=160, device=0, lib=side.lib)
    al = api.Aligner(ix, api.default_opts(side.lib, batch_pairs=300), max_pairs=1024, emit=api.EMIT_SAM, tuning=BINNED)
    sam = [ix.sam_header()]
    while True:
        n, b = fe.next()
        if n <= 0:
            break
        al.align_text(b)
        sam.append(al.sam_text())
        fe.release(b)
    gs = al.stats()
    fe.close(); al.close(); ix.close()
    assert n == 0
    assert b"".join(sam) == sam_want
    assert gs["filter_probes"] == oc["filter_probes"] and gs["filter_binned_reads"] == 1200


@pytest.mark.gpu
def test_text_batch_through_the_binned_filter_gpu(gpu_side, refs, tmp_path):
    text_batch(gpu_side, refs, tmp_path)


# ---- two contexts of one device: the shared scratch under the chain ----------------------------------------------------------------------
def two_contexts(side, golden_cases):
    """two streams inside the library (fq_stream_run), both filtering in the binned form: every call's SAM text is the one the same
    context gives when the calls are made one by one"""
    per_stream, want = [], []
    ix = None
    for tag in ("basic", "qc"):
        g = golden_cases[tag]
        names, seq, qual, lens = ob.read_fastq_pair(g["fq1"], g["fq2"])
        if ix is None or ix.prefix != g["prefix"]:
            ix = side.index(g["prefix"])
        B, n = g["batch"], seq.shape[1]
        packs = [api.HostPacked(seq[:, a:a + B], qual[:, a:a + B], lens[:, a:a + B], names[a:a + B], lib=side.lib) for a in range(0, n, B)][:3]
        al = api.Aligner(ix, api.default_opts(side.lib, trim_qual=g["trim_qual"]), max_pairs=max(16, B), tuning={"filter_binned_min": 1 << 30})
        sams = []
        for p in packs:
            al.align_packed(p)
            sams.append(al.sam_text())
        al.close()
        want.append(sams)
        per_stream.append((ix, g, packs))
    aligners = [api.Aligner(ix_, api.default_opts(side.lib, trim_qual=g_["trim_qual"]), max_pairs=max(16, g_["batch"]), tuning=BINNED) for ix_, g_, _ in per_stream]
    got = [[None] * len(p) for _, _, p in per_stream]

    def on_call(stream, call):
        if call < len(got[stream]):
            got[stream][call] = aligners[stream].sam_text()
    n_calls = min(len(p) for _, _, p in per_stream)
    api.stream_run(aligners, [p for _, _, p in per_stream], n_calls, on_call=on_call, lib=side.lib)
    for s in range(2):
        assert got[s][:n_calls] == want[s][:n_calls], "stream %d" % s
        assert aligners[s].stats()["filter_binned_reads"] > 0
    for al in aligners:
        al.close()
    for _, _, packs in per_stream:
        for p in packs:
            p.free()


@pytest.mark.gpu
def test_two_contexts_share_the_scratch_gpu(gpu_side, golden_cases):
    two_contexts(gpu_side, golden_cases)


def test_two_contexts_share_the_scratch_host_loops(emu_side, golden_cases):
    two_contexts(emu_side, golden_cases)
