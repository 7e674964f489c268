"""pop+con: the contamination and ancestry estimate (`FASTQuick_amd pop+con`, fq_popcon_*) against goldens made by the real
VerifyBamID2 ContaminationEstimator (tests/golden/_popcon/README.md says how).

CPU tier: the host evaluator (--host_eval) is the reference's arithmetic restated, so the likelihood at the golden points, the estimates and the
three output files are held to the goldens bit for bit and byte for byte; the readers' quirks and the refusals; tests/popcon_check runs the host
side under ASan / UBSan as a program of its own.  GPU tier: the kernels against the same goldens within DEVICE_LLK_BOUND, determinism, and the
estimate end to end within the reference's own slack at its stopping rule."""
from __future__ import annotations

import atexit
import functools
import os
import shutil
import subprocess
import sys
import tarfile
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fastquick_amd import api  # noqa: E402

# tests/golden/_popcon (the leading underscore: tests/golden_util.py takes every other directory there for an alignment case): cases.txt and the recorded
# numbers <case>.golden as plain files; the inputs (.UD / .mu / .bed / .af, pileups) and the reference's output files in fixtures.tar.gz, unpacked when
# a test first asks for one of them
GOLD = os.path.join(ROOT, "tests", "golden", "_popcon")


@functools.lru_cache(maxsize=None)
def data_dir():
    d = tempfile.mkdtemp(prefix="popcon_golden_")
    atexit.register(shutil.rmtree, d, True)
    with tarfile.open(os.path.join(GOLD, "fixtures.tar.gz")) as tar:
        tar.extractall(d)
    return d


def data(name):
    return os.path.join(data_dir(), name)


class _Cases(dict):      # (the paths of a case's inputs are made when the case is looked up)
    def __getitem__(self, k):
        c = dict.__getitem__(self, k)
        return dict(c, svd=data(c["svd"]), pileup=data(c["pileup"]))


CLI = os.path.join(ROOT, "fastquick_amd", "bin", "FASTQuick_amd")
CHECK_DIR = os.path.join(ROOT, "tests", "popcon_check")
# Worst relative difference device-vs-golden measured over every fixture and point (profiles/popcon.txt): 2.79e-15 -- the device library's exp / log /
# pow against glibc's, a few ulp per term, and the reduction's order.  The bound is 8 x that; it may in no case exceed 1e-9: one misclassified base
# or one wrongly skipped marker moves these fixtures' sums by more than 1e-7 relative.
DEVICE_LLK_BOUND = 8 * 2.79e-15
assert DEVICE_LLK_BOUND <= 1e-9


def _cases():
    out = _Cases()
    with open(os.path.join(GOLD, "cases.txt")) as f:
        for line in f:
            w = line.split()
            out[w[0]] = {"name": w[0], "svd": w[1], "pileup": w[2], "num_pc": int(w[3]), "opts": w[4:]}
    return out


CASES = _cases()
NAMES = sorted(CASES)
MIXTURES = ["mix_a", "mix_b"]


def golden(name):
    k = CASES[name]["num_pc"]
    g = {"points": [], "llk": [], "final": {}}
    with open(os.path.join(GOLD, name + ".golden")) as f:
        for line in f:
            w = line.split()
            if w[0] == "point":      # point pc1 <k> pc2 <k> alpha a llk v
                g["points"].append([float(x) for x in w[2:2 + k] + w[3 + k:3 + 2 * k] + [w[4 + 2 * k]]])
                g["llk"].append(float(w[6 + 2 * k]))
            elif w[0] == "final":      # final eps e alpha a pc1 <k> pc2 <k> llk1 v llk0 v
                g["final"][w[2]] = {"alpha": float(w[4]), "pc1": [float(x) for x in w[6:6 + k]], "pc2": [float(x) for x in w[7 + k:7 + 2 * k]],
                                    "llk1": float(w[8 + 2 * k]), "llk0": float(w[10 + 2 * k])}
            else:
                g[w[0]] = float(w[1])
    assert len(g["points"]) >= 6 and set(g["final"]) == {"1e-08", "1e-10"}
    return g


def estimator(name, host_eval, epsilon=1e-8, pileup=None):
    c = CASES[name]
    kw = {}
    for o in c["opts"]:
        if o == "within":
            kw["within_ancestry"] = True
        elif o == "nosanity":
            kw["disable_sanity_check"] = True
        elif o.startswith("fixpc="):
            kw["fix_pc"] = [float(x) for x in o[6:].split(":")]
        elif o.startswith("fixalpha="):
            kw["fix_alpha"] = float(o[9:])
        elif o.startswith("knownaf="):
            kw["known_af"] = data(o[8:])
    e = api.Popcon(svd_prefix=c["svd"], num_pc=c["num_pc"], host_eval=host_eval, epsilon=epsilon, **kw)
    e.set_pileup_file(pileup or c["pileup"])
    return e


def cli_flags(name):
    c = CASES[name]
    out = ["--SVDPrefix", c["svd"], "--PileupFile", c["pileup"], "--NumPC", str(c["num_pc"])]
    for o in c["opts"]:
        if o == "within":
            out.append("--WithinAncestry")
        elif o == "nosanity":
            out.append("--DisableSanityCheck")
        elif o.startswith("fixpc="):
            out += ["--FixPC", o[6:]]
        elif o.startswith("fixalpha="):
            out += ["--FixAlpha", o[9:]]
        elif o.startswith("knownaf="):
            out += ["--KnownAF", data(o[8:])]
    return out


def bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


def read(path):
    with open(path, "rb") as f:
        return f.read()


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_llk_equals_golden_bits(name):
    g = golden(name)
    e = estimator(name, host_eval=True)
    try:
        one = [e.llk(p)[0] for p in g["points"]]
        many = e.llk(g["points"])
    finally:
        e.close()
    assert bits(one) == bits(g["llk"]), (one, g["llk"])
    assert bits(many) == bits(g["llk"])


@pytest.mark.parametrize("name", NAMES)
def test_host_estimate_equals_golden_bits(name):
    g = golden(name)
    for eps in (1e-8, 1e-10):
        e = estimator(name, host_eval=True, epsilon=eps)
        try:
            r = e.run()
        finally:
            e.close()
        f = g["final"]["%g" % eps]
        got = [r["alpha"]] + r["pc1"] + r["pc2"] + [r["llk1"], r["llk0"]]
        want = [f["alpha"]] + f["pc1"] + f["pc2"] + [f["llk1"], f["llk0"]]
        assert bits(got) == bits(want), (eps, got, want)
        assert bits(r["avg_depth"]) == bits(g["avg_depth"]) and bits(r["sd_depth"]) == bits(g["sd_depth"])
        assert r["n_marker"] == g["num_marker"]


@pytest.mark.parametrize("name", NAMES)
def test_cli_host_eval_writes_golden_bytes(name, tmp_path):
    out = str(tmp_path / "o")
    run = subprocess.run([CLI, "pop+con", "--Output", out, "--host_eval"] + cli_flags(name), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    for ext in (".selfSM", ".Ancestry", ".Summary"):
        assert read(out + ext) == read(data(name + ext)), ext


def test_swap_case_swaps():
    """alpha lands at 0.7: components 1 and 2 of the two samples are exchanged, FREEMIX is folded"""
    f = golden("swap")["final"]["1e-08"]
    assert f["alpha"] >= 0.5
    assert b"Contamination Level : 0.3\n" == read(data("swap.Summary"))
    # ... and an alpha the minimiser itself drives above 0.5 (the intended sample's PCs fixed at the contaminant's): the estimate is folded
    f = golden("swapfree")["final"]["1e-08"]
    assert 0.9 < f["alpha"] < 0.95 and f["pc1"] == [-0.028, 0.012]
    assert b"Contamination Level : 0.0801744\n" == read(data("swapfree.Summary"))


def test_summary_line_is_appended(tmp_path):
    out = str(tmp_path / "o")
    with open(out + ".Summary", "w") as f:
        f.write("Statistics : kept\n")
    subprocess.run([CLI, "pop+con", "--Output", out, "--host_eval"] + cli_flags("edge"), check=True, stderr=subprocess.DEVNULL, timeout=300)
    assert read(out + ".Summary") == b"Statistics : kept\n" + read(data("edge.Summary"))


def _pileup_lines(name):
    with open(CASES[name]["pileup"]) as f:
        return f.read().splitlines(keepends=True)


def _bed(name):
    with open(CASES[name]["svd"] + ".bed") as f:
        return [l.split() for l in f]


def test_depth_column_not_string_length(tmp_path):
    """numBases adds the depth column: a line whose column says more than its strings hold moves avgDepth (and nothing else)"""
    g = golden("edge")
    lines = _pileup_lines("edge")
    n_chars = sum(len(l.split("\t")[4]) for l in lines if l.split("\t")[0] != "notachrom" and len(l.split("\t")) > 4)
    cols = sum(int(l.split("\t")[3]) for l in lines if l.split("\t")[0] != "notachrom")
    assert cols != n_chars      # (the fixture has such a line)
    e = estimator("edge", host_eval=True)
    try:
        r = e.run()
    finally:
        e.close()
    in_bed = {(b[0], b[2]) for b in _bed("edge")}
    kept = [l for l in lines if (l.split("\t")[0], l.split("\t")[1]) in in_bed]
    assert r["avg_depth"] == sum(int(l.split("\t")[3]) for l in kept) / len(kept) == g["avg_depth"]


def test_duplicate_sites_are_merged(tmp_path):
    """two lines of a site count as two lines (effectiveNumSite) and one marker with the bases of both, in file order"""
    bed = _bed("edge")
    pt = golden("edge")["points"][3]
    a, b = str(tmp_path / "a.pileup"), str(tmp_path / "b.pileup")
    with open(a, "w") as f:
        f.write("%s\t%s\t%s\t2\t.%s\tI5\n" % (bed[3][0], bed[3][2], bed[3][3], bed[3][4]) + "%s\t%s\t%s\t1\t,\t?\n" % (bed[9][0], bed[9][2], bed[9][3]) +
                "%s\t%s\t%s\t2\t,N\t+~\n" % (bed[3][0], bed[3][2], bed[3][3]))
    with open(b, "w") as f:
        f.write("%s\t%s\t%s\t4\t.%s,N\tI5+~\n" % (bed[3][0], bed[3][2], bed[3][3], bed[3][4]) + "%s\t%s\t%s\t1\t,\t?\n" % (bed[9][0], bed[9][2], bed[9][3]))
    vals = []
    for path in (a, b):
        e = estimator("edge", host_eval=True, pileup=path)
        try:
            vals.append(e.marker_llk(pt, len(bed)))
        finally:
            e.close()
    assert bits(vals[0]) == bits(vals[1]) and vals[0][3] != 0 and vals[0][9] != 0 and np.count_nonzero(vals[0]) == 2


def test_pileup_arrays_equal_the_pileup_file():
    """fq_popcon_set_pileup_arrays: the edge fixture's bases handed over in memory give the file's per-marker values and estimate"""
    row = {}
    for i, b in enumerate(_bed("edge")):
        row.setdefault((b[0], b[2]), i)
    marker, base, qual = [], [], []
    for l in _pileup_lines("edge"):
        w = l.rstrip("\n").split("\t")
        if (w[0], w[1]) in row:
            marker += [row[(w[0], w[1])]] * len(w[4])
            base += list(w[4].encode())
            qual += list(w[5].encode())
    pt = golden("edge")["points"][4]
    f, a = estimator("edge", host_eval=True), estimator("edge", host_eval=True)
    try:
        a.set_pileup_arrays(marker, base, qual)
        assert bits(a.marker_llk(pt, len(row))) == bits(f.marker_llk(pt, len(row)))
        ra, rf = a.run(), f.run()
        assert bits([ra["alpha"], ra["llk1"], ra["llk0"]] + ra["pc1"] + ra["pc2"]) == bits([rf["alpha"], rf["llk1"], rf["llk0"]] + rf["pc1"] + rf["pc2"])
        assert ra["avg_depth"] == len(marker) / len(set(marker))      # numBases is the number of bases, a site is a marker that has one
        with pytest.raises(api.FastquickError, match="no base"):      # an empty pileup is refused, not run
            a.set_pileup_arrays([], [], [])
    finally:
        f.close()
        a.close()


def test_missing_ref_allele_with_dotted_bases_ends_the_run(tmp_path):
    bed = _bed("edge")
    path = str(tmp_path / "p.pileup")
    with open(path, "w") as f:
        f.write("%s\t%s\t.\t2\t.,\tII\n" % (bed[0][0], bed[0][2]))
    with pytest.raises(api.FastquickError, match="cannot find ref allele"):
        estimator("edge", host_eval=True, pileup=path)
    with open(path, "w") as f:      # (letters alone under ref "." are read)
        f.write("%s\t%s\t.\t2\t%s%s\tII\n" % (bed[0][0], bed[0][2], bed[0][4], bed[0][4]))
    estimator("edge", host_eval=True, pileup=path).close()


def _cli_refused(args):
    run = subprocess.run([CLI, "pop+con"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode != 0
    return run.stderr.decode()


def test_cli_refusals(tmp_path):
    out = str(tmp_path / "o")
    base = ["--Output", out, "--host_eval"]
    assert "only permits as large as 4" in _cli_refused(base + [f if f != "2" else "5" for f in cli_flags("edge")])
    assert "--PileupFile" in _cli_refused(base + ["--SVDPrefix", CASES["edge"]["svd"], "--BamFile", "x.bam"])
    assert "--PileupFile" in _cli_refused(base + ["--RefVCF", "x.vcf"])
    # the between-ancestry model with one component (the reference indexes component 2 there)
    assert "--WithinAncestry" in _cli_refused(base + ["--SVDPrefix", CASES["edge"]["svd"], "--PileupFile", CASES["edge"]["pileup"], "--NumPC", "1"])
    # a sanity check that fails: 130 markers are not "> 1000"
    err = _cli_refused(base + [f for f in cli_flags("edge") if f != "--DisableSanityCheck"])
    assert "Insufficient Available markers" in err
    assert not os.path.exists(out + ".selfSM")


def test_accepted_and_ignored_flags(tmp_path):
    out = str(tmp_path / "o")
    run = subprocess.run([CLI, "pop+con", "--Output", out, "--host_eval", "--Seed", "7", "--NumThread", "3", "--Reference", "none.fa"] + cli_flags("edge"), stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0 and run.stderr.count(b"accepted and ignored") == 3
    assert read(out + ".selfSM") == read(data("edge.selfSM"))


def test_host_side_under_sanitizers(tmp_path):
    """tests/popcon_check: readers, host evaluator, minimiser and writers over the edge fixture, ASan + UBSan, a program of its own"""
    subprocess.check_call(["make", "-s", "-C", CHECK_DIR, "popcon_check"])
    out = str(tmp_path / "o")
    c = CASES["edge"]
    run = subprocess.run([os.path.join(CHECK_DIR, "popcon_check"), c["svd"], c["pileup"], os.path.join(GOLD, "edge.golden"), str(c["num_pc"]), out],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert run.returncode == 0, run.stderr.decode()[-3000:]
    assert b"0 differ" in run.stdout and b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr
    for ext in (".selfSM", ".Ancestry", ".Summary"):
        assert read(out + ext) == read(data("edge" + ext))


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.gpu
@pytest.mark.parametrize("n_points", [1, 7])
def test_device_llk_against_golden(n_points):
    worst = 0.0
    for name in NAMES:
        g = golden(name)
        e = estimator(name, host_eval=False)
        try:
            if n_points == 1:
                got = [e.llk(p)[0] for p in g["points"]]
                want = g["llk"]
            else:
                got, want = list(e.llk(g["points"][:7])) + list(e.llk(g["points"][-7:])), g["llk"][:7] + g["llk"][-7:]
        finally:
            e.close()
        w = max(rel(a, b) for a, b in zip(got, want))
        print("device llk, P = %d, %s: worst relative difference %.3g" % (n_points, name, w))
        worst = max(worst, w)
    print("device llk, P = %d: worst relative difference over all fixtures %.3g (bound %.3g)" % (n_points, worst, DEVICE_LLK_BOUND))
    assert worst <= DEVICE_LLK_BOUND


@pytest.mark.gpu
def test_device_llk_is_deterministic_and_per_marker_values_hold():
    g = golden("edge")
    n = int(g["num_marker"])
    d = estimator("edge", host_eval=False)
    h = estimator("edge", host_eval=True)
    try:
        a, b = d.llk(g["points"][:7]), d.llk(g["points"][:7])
        assert bits(a) == bits(b)
        assert bits(d.llk(g["points"][2])) == bits(d.llk(g["points"][2])) == bits(a[2:3])      # (a point's value does not depend on its place in a batch)
        for pt in g["points"][:3]:
            dm, dm2, hm = d.marker_llk(pt, n), d.marker_llk(pt, n), h.marker_llk(pt, n)
            assert bits(dm) == bits(dm2)
            for i in (63, 64, 65):      # depths 63, 64, 65: around four whole sixteen-byte pieces
                assert hm[i] != 0
                print("marker %d: device %.17g host %.17g (relative difference %.3g)" % (i, dm[i], hm[i], rel(dm[i], hm[i])))
                assert rel(dm[i], hm[i]) <= DEVICE_LLK_BOUND
            assert np.array_equal(dm == 0, hm == 0)      # the skipped, the absent and the underflowing markers are the same ones
            assert hm[5] == 0 and hm[6] == 0 and hm[71] == 0
    finally:
        d.close()
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", MIXTURES)
def test_device_estimate_end_to_end(name):
    """alpha and every PC within 4 x |golden(1e-8) - golden(1e-10)| -- the reference's own slack at its stopping rule; FREELK1 / FREELK0 through the
    device likelihood at the golden's point"""
    g = golden(name)
    f8, f10 = g["final"]["1e-08"], g["final"]["1e-10"]
    e = estimator(name, host_eval=False)
    try:
        r = e.run()
    finally:
        e.close()
    got = [r["alpha"]] + r["pc1"] + r["pc2"]
    w8 = [f8["alpha"]] + f8["pc1"] + f8["pc2"]
    w10 = [f10["alpha"]] + f10["pc1"] + f10["pc2"]
    labels = ["alpha"] + ["pc1[%d]" % i for i in range(len(r["pc1"]))] + ["pc2[%d]" % i for i in range(len(r["pc2"]))]
    for lab, a, b8, b10 in zip(labels, got, w8, w10):
        print("%s %s: device %.10g golden %.10g distance %.3g allowed %.3g" % (name, lab, a, b8, abs(a - b8), 4 * abs(b8 - b10)))
    print("%s: %d evaluations, llk1 %.17g (golden %.17g)" % (name, r["n_eval"], r["llk1"], f8["llk1"]))
    e = estimator(name, host_eval=False)
    try:
        at = e.llk([f8["pc1"] + f8["pc2"] + [f8["alpha"]], f8["pc1"] + f8["pc1"] + [0.0]])
    finally:
        e.close()
    print("%s: FREELK1 at the golden's point %.17g (golden %.17g), FREELK0 %.17g (golden %.17g)" % (name, at[0], -f8["llk1"], at[1], -f8["llk0"]))
    assert rel(at[0], -f8["llk1"]) <= DEVICE_LLK_BOUND and rel(at[1], -f8["llk0"]) <= DEVICE_LLK_BOUND
    for lab, a, b8, b10 in zip(labels, got, w8, w10):
        assert abs(a - b8) <= 4 * abs(b8 - b10), lab


@pytest.mark.gpu
def test_cli_device_writes_the_files(tmp_path):
    out = str(tmp_path / "o")
    run = subprocess.run([CLI, "pop+con", "--Output", out] + cli_flags("mix_b"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    assert b"device kernels" in run.stderr
    want = read(data("mix_b.selfSM")).split(b"\n")
    got = read(out + ".selfSM").split(b"\n")
    assert got[0] == want[0] and got[1].split(b"\t")[:6] == want[1].split(b"\t")[:6]
    assert read(out + ".Ancestry").startswith(b"PC\tContaminatingSample\tIntendedSample\n1\t")


# ---- `align --popcon_svd` ------------------------------------------------------------------------------------------------------------------------
QC_FILES = ["InsertSizeTable", "DepthDist", "GCDist", "EmpRepDist", "EmpCycleDist", "RawInsertSizeDist", "SexChromInfo", "Pileup", "FASTQ.csv", "Sequence.csv", "Summary",
            "AdjustedInsertSizeDist", "vcf"]


def pileup_records(blob: bytes):
    """the lines of an O.Pileup file: chrom, pos, '.', depth, bases, qualities, mapping qualities (raw bytes: a tab or a line end may be among them), cycles"""
    p = 0
    while p < len(blob):
        f = []
        for _ in range(4):
            q = blob.index(b"\t", p)
            f.append(blob[p:q])
            p = q + 1
        d = int(f[3])
        bases, quals, maq = blob[p:p + d], blob[p + d + 1:p + 2 * d + 1], blob[p + 2 * d + 2:p + 3 * d + 2]
        assert blob[p + d] == blob[p + 2 * d + 1] == blob[p + 3 * d + 2] == 9
        p = blob.index(b"\n", p + 3 * d + 3) + 1
        yield f[0].decode(), int(f[1]), bases, quals, maq


def convert_pileup(pileup_path, bed_path, out_path):
    """what `align --popcon_svd` hands over, as a pileup file: sites of the .bed, a base equal to the ref allele as '.' / ',' by strand, entries with a mapping
    quality below 13 or a base quality below 2 left out, sites that keep no base left out"""
    ref_of = {}
    with open(bed_path) as f:
        for line in f:
            w = line.split()
            ref_of[(w[0], int(w[2]))] = w[3]
    n = 0
    with open(out_path, "wb") as out:
        for chrom, pos, bases, quals, maq in pileup_records(read(pileup_path)):
            if (chrom, pos) not in ref_of:
                continue
            r = ord(ref_of[(chrom, pos)].upper())
            keep = [t for t in range(len(bases)) if maq[t] >= 13 and quals[t] - 33 >= 2]
            if not keep:
                continue
            b = bytes((ord(".") if bases[t] < 97 else ord(",")) if (bases[t] & ~32) == r else bases[t] for t in keep)
            out.write(b"%s\t%d\t%s\t%d\t%s\t%s\n" % (chrom.encode(), pos, ref_of[(chrom, pos)].encode(), len(keep), b, bytes(quals[t] for t in keep)))
            n += 1
    return n


@pytest.mark.gpu
def test_align_popcon_svd_equals_pop_con_on_the_converted_pileup(tmp_path):
    from fastquick_amd import synth
    ref = synth.make_reference(n_markers=1100, n_long=60, seed=901)
    pre = str(tmp_path / "ref.FASTQuick.fa")
    ref.write_fasta(pre)
    api.build_index(pre)
    synth.write_qc_inputs(pre, ref)
    synth.write_param(pre, ref, 60)
    with open(pre + ".genome.fa.fai", "w") as fh:
        fh.write("1\t%d\t3\t60\t61\n" % len(ref.genome))
    rb = synth.make_reads(ref, 24000, on_target=1.0, seed=902, sub_rate=0.01)
    fq = []
    for e in range(2):
        fq.append(str(tmp_path / ("r_%d.fq.gz" % (e + 1))))
        synth.write_fastq_uniform(rb.seq[e], rb.qual[e], 150, fq[e], threads=4)
    # .UD / .mu / .bed of the marker set: our own random numbers, three of the markers left out, one row of a site the run has no marker at
    rng = np.random.default_rng(903)
    svd = str(tmp_path / "svd")
    with open(svd + ".UD", "w") as fu, open(svd + ".mu", "w") as fm, open(svd + ".bed", "w") as fb:
        for k, nm in enumerate(ref.names):
            if k in (5, 500, 1099):
                continue
            chrom, rest = nm.split(":")
            pos = int(ref.marker_pos[k])
            r, a = rest.split("@")[1].split("|")[0].split("/")
            if k == 700:
                pos, r = pos + 7, "A"
            fu.write("\t".join("%.6g" % x for x in rng.normal(0, 2.0, 4)) + "\t\n")
            fm.write("%s:%d\t%.5f\n" % (chrom, pos, rng.uniform(0.05, 1.9)))
            fb.write("%s\t%d\t%d\t%s\t%s\n" % (chrom, pos - 1, pos, r, a))
    outs = {}
    for mode, extra in (("plain", []), ("popcon", ["--popcon_svd", svd, "--popcon_numpc", "2"])):
        out = str(tmp_path / mode)
        cmd = [CLI, "align", "--index_prefix", pre[:-len(".FASTQuick.fa")], "--fastq_1", fq[0], "--fastq_2", fq[1], "--out_prefix", out, "--read_len", "151"] + extra
        run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert run.returncode == 0, run.stderr.decode(errors="replace")[-2500:]
        outs[mode] = {f: read(out + "." + f).replace(out.encode(), b"OUT") for f in QC_FILES + ["bam"]}
        outs[mode]["vcf"] = b"\n".join(ln for ln in outs[mode]["vcf"].split(b"\n") if not ln.startswith(b"##fileDate="))
    assert not os.path.exists(str(tmp_path / "plain") + ".selfSM") and not os.path.exists(str(tmp_path / "plain") + ".Ancestry")
    for f in QC_FILES + ["bam"]:
        if f != "Summary":
            assert outs["plain"][f] == outs["popcon"][f], f
    tail = outs["popcon"]["Summary"][len(outs["plain"]["Summary"]):]
    assert outs["popcon"]["Summary"].startswith(outs["plain"]["Summary"]) and tail.startswith(b"Contamination Level : ") and tail.count(b"\n") == 1
    conv = str(tmp_path / "conv.pileup")
    assert convert_pileup(str(tmp_path / "popcon") + ".Pileup", svd + ".bed", conv) > 1000
    out = str(tmp_path / "file")
    run = subprocess.run([CLI, "pop+con", "--PileupFile", conv, "--SVDPrefix", svd, "--NumPC", "2", "--Output", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-2500:]
    assert read(out + ".selfSM") == read(str(tmp_path / "popcon") + ".selfSM")
    assert read(out + ".Ancestry") == read(str(tmp_path / "popcon") + ".Ancestry")
    assert read(out + ".Summary") == tail
