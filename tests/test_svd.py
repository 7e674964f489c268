"""svd: the SVD files of a reference panel (`FASTQuick_amd svd --RefVCF`, fq_svd_*) against goldens made by the real VerifyBamID2
SVDcalculator::ProcessRefVCF (tests/golden/_svd/README.md says how).

The reader and the writers are held to the goldens byte for byte (.mu, .bed).  The decomposition has no tolerance chosen in advance: T is numpy's float64
SVD of the centred matrix X (genotypes minus the float means); per component, with the sign aligned by the dot product of the V columns, e_ref is the
largest distance of the golden's printed column from T and e_ours that of the ABI's doubles, for V and for UD; the test asserts e_ours <= e_ref for all
ten components -- at least as close to the true decomposition as the reference's own files -- and, on the goldens alone, e_ref <= 1e-4 (V) and
e_ref <= 1e-4 max|UD| (UD), so that a near-degenerate fixture cannot make the comparison empty.

CPU tier: the host loops (--host_eval) through the ABI and the command line, the refusals, tests/svd_check under ASan / UBSan as a program of its own.
GPU tier: the Gram kernel against numpy's integer product (the check of the i8 matrix instruction's operand lanes), the device decomposition under the
same criterion, determinism, the command line, and pop+con on the written prefix."""
from __future__ import annotations

import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fastquick_amd import api  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "_svd")
CLI = os.path.join(ROOT, "fastquick_amd", "bin", "FASTQuick_amd")
CHECK_DIR = os.path.join(ROOT, "tests", "svd_check")
SHAPES = ["p333x45", "p640x96", "p97x33", "p40x16"]
GRAM_SHAPES = [(1, 10), (31, 33), (32, 32), (33, 31), (64, 65), (97, 33), (333, 45), (640, 96)]


def vcf_of(name):
    return os.path.join(GOLD, "edge.vcf" if name == "edge" else name + ".vcf.gz")


def read(path):
    with open(path, "rb") as f:
        return f.read()


def parse_table(path, skip):
    """the values of a .UD (skip 0) or .V (skip 1: the sample name) file, and its tokens as text"""
    rows = [line.rstrip("\n").split("\t") for line in open(path)]
    assert all(len(r) == skip + 11 and r[-1] == "" for r in rows), path      # ten values, each followed by a tab
    text = [r[skip:skip + 10] for r in rows]
    return np.array(text, dtype=np.float64), text


@functools.lru_cache(maxsize=None)
def panel(name):
    """the genotypes SVDcalculator::ReadVcf keeps, read here from the fixture's own text (GT, PL or GL records as synth.panel_vcf writes them)"""
    rows = []
    with gzip.open(vcf_of(name), "rt") as f:
        for line in f:
            if line.startswith("#"):
                continue
            w = line.rstrip("\n").split("\t")
            keys = w[8].split(":")
            key = "PL" if "PL" in keys else "GL" if "GL" in keys else "GT"
            row = []
            for cell in w[9:]:
                v = cell.split(":")[keys.index(key)]
                if key == "GT":
                    s = sum(0 if a == "." else int(a) for a in v.replace("|", "/").split("/"))
                    ph = (0, 30, 50) if s == 0 else (50, 0, 50) if s == 1 else (50, 30, 0)
                elif key == "PL":
                    ph = tuple(int(x) for x in v.split(","))
                else:
                    ph = tuple(int(-10.0 * float(x)) for x in v.split(","))
                best, g = 255, -1
                for k in range(3):
                    if min(ph[k], 255) < best:
                        best, g = min(ph[k], 255), k
                row.append(g)
            rows.append(row)
    return np.array(rows, dtype=np.int8)


@functools.lru_cache(maxsize=None)
def truth(name):
    """T: numpy's float64 SVD of X = G - float means; and the golden's columns with e_ref per component"""
    G = panel(name).astype(np.float64)
    mu = (G.sum(axis=1).astype(np.float32) / np.float32(G.shape[1])).astype(np.float64)
    U, S, Vt = np.linalg.svd(G - mu[:, None], full_matrices=False)
    T = {"v": Vt[:10].T.copy(), "ud": U[:, :10] * S[:10], "sigma": S, "mu": mu}
    gold = {"v": parse_table(os.path.join(GOLD, name + ".V"), 1)[0], "ud": parse_table(os.path.join(GOLD, name + ".UD"), 0)[0]}
    T["e_ref"] = errors(T, gold["v"], gold["ud"])
    for a in T.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return T


def errors(T, v, ud):
    """per component the largest distance of a column of v and of ud from T's, the sign aligned by the dot product of the V columns"""
    ev, eu = [], []
    for c in range(10):
        s = 1.0 if float(v[:, c] @ T["v"][:, c]) >= 0 else -1.0
        ev.append(float(np.abs(s * v[:, c] - T["v"][:, c]).max()))
        eu.append(float(np.abs(s * ud[:, c] - T["ud"][:, c]).max()))
    return {"v": ev, "ud": eu}


def assert_criterion(name, r, label):
    T = truth(name)
    ours = errors(T, r["v"], r["ud"])
    for c in range(10):
        print("%s %s component %d: V e_ours %.3g e_ref %.3g; UD e_ours %.3g e_ref %.3g" % (label, name, c, ours["v"][c], T["e_ref"]["v"][c], ours["ud"][c], T["e_ref"]["ud"][c]))
    for c in range(10):
        assert ours["v"][c] <= T["e_ref"]["v"][c], (name, "V", c, ours["v"][c], T["e_ref"]["v"][c])
        assert ours["ud"][c] <= T["e_ref"]["ud"][c], (name, "UD", c, ours["ud"][c], T["e_ref"]["ud"][c])
    assert np.array_equal(r["mu"], T["mu"])
    for c in range(10):      # the stated sign: the entry of largest magnitude positive
        assert r["v"][np.argmax(np.abs(r["v"][:, c])), c] > 0


def decompose(name, host_eval, prefix=None):
    s = api.Svd(host_eval=host_eval)
    try:
        s.read_vcf(vcf_of(name))
        r = s.run()
        if prefix:
            s.write(prefix)
    finally:
        s.close()
    return r


def assert_text_is_percent_g(prefix, r):
    """each printed value is '%g' of the double (default ostream formatting)"""
    for ext, key, skip in ((".UD", "ud", 0), (".V", "v", 1)):
        text = parse_table(prefix + ext, skip)[1]
        want = [["%g" % x for x in row] for row in r[key]]
        assert text == want, ext


# ---- the fixtures themselves -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_fixture_is_not_degenerate(name):
    T = truth(name)
    scale = float(np.abs(T["ud"]).max())
    for c in range(10):
        print("%s component %d: e_ref V %.3g, UD %.3g (max|UD| %.3g), sigma ratio %.4f" % (name, c, T["e_ref"]["v"][c], T["e_ref"]["ud"][c], scale, T["sigma"][c + 1] / T["sigma"][c]))
        assert T["e_ref"]["v"][c] <= 1e-4
        assert T["e_ref"]["ud"][c] <= 1e-4 * scale


# ---- CPU tier --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES + ["edge"])
def test_mu_and_bed_equal_golden_bytes(name, tmp_path):
    out = str(tmp_path / "o")
    decompose(name, True, out)
    for ext in (".mu", ".bed"):
        assert read(out + ext) == read(os.path.join(GOLD, name + ext)), ext
    with open(out + ".V") as f:
        names = [line.split("\t")[0] for line in f]
    with open(os.path.join(GOLD, name + ".V")) as f:
        assert names == [line.split("\t")[0] for line in f]


def test_plain_gzip_and_bgzf_give_the_same_files(tmp_path):
    from fastquick_amd import synth
    text = gzip.open(vcf_of("p97x33"), "rb").read()
    forms = {"plain": text, "bgzf": synth.bgzf_compress(text, threads=2, level=6, member=3000)}      # (several BGZF members)
    decompose("p97x33", True, str(tmp_path / "gz"))
    for form, data in forms.items():
        path = str(tmp_path / (form + ".vcf"))
        with open(path, "wb") as f:
            f.write(data)
        s = api.Svd(host_eval=True)
        try:
            s.read_vcf(path)
            s.run()
            s.write(str(tmp_path / form))
        finally:
            s.close()
        for ext in (".mu", ".bed", ".UD", ".V"):
            assert read(str(tmp_path / form) + ext) == read(str(tmp_path / "gz") + ext), (form, ext)


@pytest.mark.parametrize("name", SHAPES)
def test_host_result_meets_the_criterion(name, tmp_path):
    out = str(tmp_path / "o")
    r = decompose(name, True, out)
    print("%s: %d iterations, residual %.3g" % (name, r["iterations"], r["residual"]))
    assert_criterion(name, r, "host")
    assert_text_is_percent_g(out, r)
    assert np.allclose(r["sigma"], truth(name)["sigma"][:10], rtol=1e-9, atol=0)


@pytest.mark.parametrize("name", SHAPES)
def test_cli_host_eval_writes_the_abi_values(name, tmp_path):
    vcf = str(tmp_path / os.path.basename(vcf_of(name)))      # --Output defaults to the VCF's path
    with open(vcf, "wb") as f:
        f.write(read(vcf_of(name)))
    args = [CLI, "svd", "--RefVCF", vcf, "--host_eval"] + ([] if name == "p40x16" else ["--Output", str(tmp_path / "o")])
    run = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    assert b"host loops" in run.stderr and b"Success!" in run.stderr
    out = vcf if name == "p40x16" else str(tmp_path / "o")
    r = decompose(name, True)
    assert_criterion(name, r, "cli")
    assert_text_is_percent_g(out, r)
    for ext in (".mu", ".bed"):
        assert read(out + ext) == read(os.path.join(GOLD, name + ext)), ext


def _vcf(path, records, n_samples=10, fmt="GT"):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + "".join("\tS%d" % j for j in range(n_samples)) + "\n")
        for chrom, pos, cells in records:
            f.write("%s\t%d\t.\tA\tC\t.\tPASS\t.\t%s\t%s\n" % (chrom, pos, fmt, "\t".join(cells)))


def _refused(path, tmp_path):
    out = str(tmp_path / "refused")
    run = subprocess.run([CLI, "svd", "--RefVCF", path, "--Output", out, "--host_eval"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode != 0
    assert not any(os.path.exists(out + ext) for ext in (".mu", ".bed", ".UD", ".V"))
    return run.stderr.decode()


def test_refusals(tmp_path):
    gt = ["0/0", "0/1", "1/1"]
    cells = lambda i, n=10: [gt[(i * 7 + j * 3) % 3] for j in range(n)]      # noqa: E731
    ok = [("1", 100 + 10 * i, cells(i)) for i in range(12)]
    p = str(tmp_path / "t.vcf")
    _vcf(p, [(c, q, x[:9]) for c, q, x in ok], n_samples=9)
    assert "and 9 samples" in _refused(p, tmp_path)                          # 9 samples
    _vcf(p, ok[:9] + [("X", 5, cells(1))])
    assert "9 markers kept" in _refused(p, tmp_path)                         # 9 kept markers (and one on X)
    _vcf(p, ok[:5] + [ok[4]] + ok[5:])
    assert "Duplicated Marker at 1:140" in _refused(p, tmp_path)             # an adjacent duplicate
    _vcf(p, [(c, q, ["30,0,%d" % (40 if (i, j) != (6, 3) else -40) for j in range(10)]) for i, (c, q, x) in enumerate(ok)], fmt="PL")
    assert "Negative PL or Positive GL observed" in _refused(p, tmp_path)    # a negative PL
    _vcf(p, [(c, q, ["7"] * 10) for c, q, x in ok], fmt="DP")
    assert "Cannot recognize GT, GL or PL key in FORMAT field" in _refused(p, tmp_path)
    _vcf(p, ok[:7] + [("1", 500, ["0/1"] * 6 + ["1"] + ["0/1"] * 3)] + ok[7:])
    err = _refused(p, tmp_path)                                              # a GT with one allele: the reference indexes out of bounds there
    assert "fewer than two alleles" in err and "line 10" in err
    _vcf(p, [(c, q, ["0,30"] * 10) for c, q, x in ok], fmt="PL")
    assert "fewer than three values" in _refused(p, tmp_path)
    assert "--RefVCF is required" in subprocess.run([CLI, "svd"], stderr=subprocess.PIPE).stderr.decode()


def test_iteration_cap_is_an_error_and_writes_nothing(tmp_path):
    s = api.Svd(host_eval=True, max_iter=1)
    try:
        s.read_vcf(vcf_of("p640x96"))
        with pytest.raises(api.FastquickError, match="did not reach"):
            s.run()
        with pytest.raises(api.FastquickError, match="nothing to write"):
            s.write(str(tmp_path / "o"))
    finally:
        s.close()
    assert not os.path.exists(str(tmp_path / "o") + ".UD")


def test_set_genotypes_equals_the_vcf(tmp_path):
    from fastquick_amd import synth
    G = panel("p97x33")
    s = api.Svd(host_eval=True)
    try:
        s.set_genotypes(G, sites=synth.panel_sites(G.shape[0]), samples=["S%04d" % j for j in range(G.shape[1])])
        assert np.array_equal(s.gram(), G.astype(np.int32).T @ G.astype(np.int32))
        s.run()
        s.write(str(tmp_path / "m"))
    finally:
        s.close()
    decompose("p97x33", True, str(tmp_path / "f"))
    for ext in (".mu", ".bed", ".UD", ".V"):
        assert read(str(tmp_path / "m") + ext) == read(str(tmp_path / "f") + ext), ext


def test_host_side_under_sanitizers(tmp_path):
    """tests/svd_check: the reader, the host loops and the writers over edge.vcf and p40x16, ASan + UBSan, a program of its own"""
    subprocess.check_call(["make", "-s", "-C", CHECK_DIR, "svd_check"])
    run = subprocess.run([os.path.join(CHECK_DIR, "svd_check"), str(tmp_path), vcf_of("edge"), vcf_of("p40x16")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert run.returncode == 0, run.stderr.decode()[-3000:]
    assert b"0 differ" in run.stdout and b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr
    for k, name in enumerate(("edge", "p40x16")):
        for ext in (".mu", ".bed"):
            assert read(str(tmp_path / str(k)) + ext) == read(os.path.join(GOLD, name + ext)), (name, ext)
    assert_text_is_percent_g(str(tmp_path / "1"), decompose("p40x16", True))


# ---- GPU tier --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,N", GRAM_SHAPES)
def test_device_gram_is_exact(M, N):
    """random genotypes, every entry drawn on its own: tiles off the diagonal are not symmetric, so a wrong operand lane map cannot hide"""
    G = np.random.default_rng(1000 * M + N).integers(-1, 3, size=(M, N)).astype(np.int8)
    s = api.Svd(host_eval=False)
    try:
        s.set_genotypes(G)
        a = s.gram()
        b = s.gram()
    finally:
        s.close()
    want = G.astype(np.int32).T @ G.astype(np.int32)
    assert np.array_equal(a, want), np.argwhere(a != want)[:5]
    assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHAPES)
def test_device_result_meets_the_criterion(name):
    r = decompose(name, False)
    print("%s: %d iterations, residual %.3g" % (name, r["iterations"], r["residual"]))
    assert_criterion(name, r, "device")


@pytest.mark.gpu
def test_device_runs_are_identical(tmp_path):
    a = decompose("p640x96", False, str(tmp_path / "a"))
    b = decompose("p640x96", False, str(tmp_path / "b"))
    assert a["ud"].tobytes() == b["ud"].tobytes() and a["v"].tobytes() == b["v"].tobytes() and a["iterations"] == b["iterations"]
    for ext in (".mu", ".bed", ".UD", ".V"):
        assert read(str(tmp_path / "a") + ext) == read(str(tmp_path / "b") + ext), ext


@pytest.mark.gpu
def test_cli_device_and_pop_con_on_the_written_prefix(tmp_path):
    out = str(tmp_path / "panel")
    run = subprocess.run([CLI, "svd", "--RefVCF", vcf_of("p333x45"), "--Output", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    assert b"device kernels" in run.stderr and b"Success!" in run.stderr
    for ext in (".mu", ".bed"):
        assert read(out + ext) == read(os.path.join(GOLD, "p333x45" + ext)), ext
    assert_text_is_percent_g(out, decompose("p333x45", False))
    # a pileup drawn over those markers: pop+con takes the prefix
    rng = np.random.default_rng(5)
    pile = str(tmp_path / "s.pileup")
    with open(out + ".bed") as fb, open(pile, "w") as fp:
        for line in fb:
            chrom, _, pos, ref, alt = line.split()
            d = int(rng.integers(4, 12))
            bases = "".join(rng.choice([".", ",", alt, alt.lower()], p=[.35, .35, .15, .15]) for _ in range(d))
            fp.write("%s\t%s\t%s\t%d\t%s\t%s\n" % (chrom, pos, ref, d, bases, "".join(rng.choice(list("5?FI")) for _ in range(d))))
    run = subprocess.run([CLI, "pop+con", "--SVDPrefix", out, "--PileupFile", pile, "--Output", str(tmp_path / "pc"), "--NumPC", "2", "--DisableSanityCheck"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    assert run.stderr.rstrip().endswith(b"Success!")
    assert os.path.exists(str(tmp_path / "pc") + ".selfSM")
