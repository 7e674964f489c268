"""svd: the chunked panel reader (fq_svd_read_panel, csrc/fq_vcf.h; `FASTQuick_amd svd --RefVCFList L --Sites S`; DESIGN.md 5v "the panel reader").

The yardsticks are the reference's own files in tests/golden/_svd and the serial reader (fq_svd_read_vcf); the chunked reader is never one.
CPU tier: reader 2, the host loops over the bodies the kernels wrap, through the ABI and the command line; tests/vcf_check under ASan / UBSan.
GPU tier: reader 1, the same checks on the device, and the shapes at which the genotype kernel can still go wrong."""
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

from fastquick_amd import api, synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "_svd")
CLI = os.path.join(ROOT, "fastquick_amd", "bin", "FASTQuick_amd")
CHECK_DIR = os.path.join(ROOT, "tests", "vcf_check")
EXTS = (".mu", ".bed", ".UD", ".V")
FIXTURES = ["p333x45", "p640x96", "p97x33", "p40x16", "edge"]
CHUNKS = [(n, c) for n in FIXTURES for c in (None, 4096)] + [("p640x96", 1024)]      # (1024: below a line's length, the chunk must grow)
HOST_LINES = {"p333x45": 0, "p640x96": 0, "p40x16": 0, "edge": 1, "p97x33": 97}      # GT / GT:PL: none; edge: the GL record; p97x33 (GL): every kept marker
HEADER = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"


def vcf_of(name):
    return os.path.join(GOLD, "edge.vcf" if name == "edge" else name + ".vcf.gz")


def read(path):
    with open(path, "rb") as f:
        return f.read()


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return path


def text_of(name):
    return read(vcf_of(name)) if name == "edge" else gzip.open(vcf_of(name), "rb").read()


def run_reader(paths, reader, tmp, sites=None, chunk=None, host_eval=True, decompose=True, tag="o"):
    """the panel, the stats and (decompose) the four files of one reader over the paths"""
    s = api.Svd(host_eval=host_eval, reader=reader, chunk_bytes=chunk)
    try:
        if reader == 0:
            s.read_vcf(paths)
        else:
            s.read_panel(paths, sites=sites)
        out = {"panel": s.panel(), "stats": s.read_stats()}
        if decompose:
            s.run()
            pre = os.path.join(str(tmp), tag)
            s.write(pre)
            out["files"] = {e: read(pre + e) for e in EXTS}
    finally:
        s.close()
    return out


def same_panel(a, b):
    return np.array_equal(a["g"], b["g"]) and a["chrom"] == b["chrom"] and np.array_equal(a["pos"], b["pos"]) and a["samples"] == b["samples"]


@functools.lru_cache(maxsize=None)
def serial(name):
    """the serial reader's panel and host-loop files of a golden fixture, computed once"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        r = run_reader(vcf_of(name), 0, tmp)
    r["panel"]["g"].setflags(write=False)
    return r


def message(fn):
    with pytest.raises(api.FastquickError) as e:
        fn()
    return str(e.value).split(": ", 1)[1]


def check_golden(name, chunk, reader, tmp_path):
    r = run_reader(vcf_of(name), reader, tmp_path, chunk=chunk)
    for ext in (".mu", ".bed"):
        assert r["files"][ext] == read(os.path.join(GOLD, name + ext)), ext
    want = serial(name)
    assert same_panel(r["panel"], want["panel"])
    for ext in EXTS:
        assert r["files"][ext] == want["files"][ext], ext
    st = r["stats"]
    print(name, chunk, st)
    assert st["host_lines"] == HOST_LINES[name] and st["kept"] == want["panel"]["g"].shape[0]
    if name == "p97x33":
        assert st["host_lines"] == st["kept"]
    if chunk == 1024:
        assert st["chunks"] > 100
    return r


# ---- the --Sites / --RefVCFList case ---------------------------------------------------------------------------------------------------------------
def snp_at_site(rec, siteset):
    """rules (a) and (b) of --Sites, stated here in Python"""
    chrom, pos, ref, alt = rec[0], rec[1], rec[2], rec[3]
    if chrom[:3] in ("chr", "CHR"):
        chrom = chrom[3:]
    return (chrom, pos) in siteset and len(ref) == 1 and any(len(a) == 1 and a in "ACGTacgt" and a.upper() != ref.upper() for a in alt.split(","))


def make_sites_case(tmp):
    """24 samples over three files (plain, gzip with chr names, BGZF), salted; the sites file shuffled with two sites the panel lacks; and the single VCF the
    serial reader gets: filtered and concatenated here"""
    rng = np.random.default_rng(11)
    N, M = 24, 66
    names = ["H%03d" % j for j in range(N)]
    G = rng.integers(0, 3, size=(M, N))
    gt = ("0/0", "0|1", "1/1")
    pl = ("0/0:0,30,50", "0/1:50,0,50", "1/1:50,30,0")
    recs, sites = [], []
    for i, (chrom, pos, ref, alt) in enumerate(synth.panel_sites(M)):
        which = 0 if int(chrom) <= 7 else 1 if int(chrom) <= 15 else 2
        cells = [(pl if which == 1 else gt)[g] for g in G[i]]
        fmt = "GT:PL" if which == 1 else "GT"
        recs.append((which, ("chr" + chrom) if which == 1 else chrom, pos, ref, alt, fmt, cells))
        if i % 3 != 1:
            sites.append((chrom, pos))                                       # (a third of the panel's records are at no site)
        if i == 5:
            recs.append((which, chrom, pos + 1, ref + "T", ref, fmt, cells)); sites.append((chrom, pos + 1))      # an indel at a site
        if i == 9:
            recs.append((which, chrom, pos + 2, ref, ref + "TT," + alt, fmt, cells)); sites.append((chrom, pos + 2))      # multi-allelic, the second ALT is the SNP
        if i == 30:
            recs.append((which, "chr" + chrom, pos + 3, ref, ".", fmt, cells)); sites.append((chrom, pos + 3))      # ALT=.
    recs.append((2, "X", 5000, "A", "C", "GT", [gt[g] for g in G[0]])); sites.append(("X", 5000))      # a site on X
    sites += [("3", 999), ("21", 123456)]                                    # two sites the panel lacks
    siteset = set(sites)
    head = HEADER + "".join("\t" + n for n in names) + "\n"
    line = lambda r: "%s\t%d\t.\t%s\t%s\t.\tPASS\t.\t%s\t%s\n" % (r[1], r[2], r[3], r[4], r[5], "\t".join(r[6]))      # noqa: E731
    texts = [(head + "".join(line(r) for r in recs if r[0] == w)).encode() for w in range(3)]
    paths = [write(os.path.join(tmp, "a.vcf"), texts[0]), write(os.path.join(tmp, "b.vcf.gz"), gzip.compress(texts[1])),
             write(os.path.join(tmp, "c.vcf.gz"), synth.bgzf_compress(texts[2], threads=2, level=6, member=3000))]
    order = rng.permutation(len(sites))
    sites_path = write(os.path.join(tmp, "sel.SelectedSite.vcf"), ("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\n" + "".join("%s%s\t%d\t.\tA\tC\n" % ("chr" if k % 5 == 0 else "", sites[k][0], sites[k][1]) for k in order)).encode())
    kept = [r for r in recs if snp_at_site(r[1:], siteset)]
    subset = write(os.path.join(tmp, "subset.vcf"), (head + "".join(line(r) for r in kept)).encode())
    hit = {((r[1][3:] if r[1][:3] == "chr" else r[1]), r[2]) for r in kept}
    lst = write(os.path.join(tmp, "panels.list"), ("\n".join(paths) + "\n").encode())
    return {"paths": paths, "sites": sites_path, "subset": subset, "list": lst, "n_sites": len(siteset), "n_found": len(hit), "n_handed": len(kept), "head": head, "line": line, "recs": recs}


def check_sites_case(reader, tmp_path):
    c = make_sites_case(str(tmp_path))
    want = run_reader(c["subset"], 0, tmp_path, tag="serial")
    got = run_reader(c["paths"], reader, tmp_path, sites=c["sites"], chunk=4096, tag="chunked")
    assert same_panel(got["panel"], want["panel"])
    for ext in EXTS:
        assert got["files"][ext] == want["files"][ext], ext
    st = got["stats"]
    print(st)
    assert st["sites"] == c["n_sites"] and st["sites_found"] == c["n_found"] and st["sites"] - st["sites_found"] == 4      # the two the panel lacks, the indel's, the ALT=. one's
    assert st["site_lines"] == c["n_handed"] and st["kept"] == want["panel"]["g"].shape[0] and st["host_lines"] == 0
    return c, want


# ---- CPU tier --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,chunk", CHUNKS)
def test_host_loops_equal_goldens_and_serial_reader(name, chunk, tmp_path):
    check_golden(name, chunk, 2, tmp_path)


def forms_of(text, tmp_path):
    return {"plain": write(str(tmp_path / "plain.vcf"), text), "gzip": write(str(tmp_path / "gz.vcf.gz"), gzip.compress(text)),
            "bgzf": write(str(tmp_path / "bgzf.vcf.gz"), synth.bgzf_compress(text, threads=2, level=6, member=3000))}


@pytest.mark.parametrize("chunk", [None, 4096])
def test_plain_gzip_and_bgzf_give_the_same_files(chunk, tmp_path):
    want = serial("p333x45")
    for form, path in forms_of(text_of("p333x45"), tmp_path).items():
        r = run_reader(path, 2, tmp_path, chunk=chunk, tag=form)
        for ext in EXTS:
            assert r["files"][ext] == want["files"][ext], (form, ext)


def test_last_line_without_line_end_and_cr_lf(tmp_path):
    text = text_of("p40x16")
    want = serial("p40x16")
    for tag, data in (("nonl", text[:-1]), ("crlf", text.replace(b"\n", b"\r\n"))):
        assert not data.endswith(b"\n") or tag == "crlf"
        for chunk in (None, 4096):
            r = run_reader(write(str(tmp_path / (tag + ".vcf")), data), 2, tmp_path, chunk=chunk, tag=tag)
            assert same_panel(r["panel"], want["panel"])
            for ext in EXTS:
                assert r["files"][ext] == want["files"][ext], (tag, chunk, ext)


def test_an_empty_line_ends_the_file(tmp_path):
    lines = text_of("p333x45").split(b"\n")
    path = write(str(tmp_path / "gap.vcf"), b"\n".join(lines[:202] + [b""] + lines[202:]))
    want = run_reader(path, 0, tmp_path, tag="serial")
    assert want["panel"]["g"].shape[0] == 200                                # (the records behind the empty line are ignored)
    for chunk in (None, 4096):
        r = run_reader(path, 2, tmp_path, chunk=chunk, tag="c")
        assert same_panel(r["panel"], want["panel"])
        for ext in EXTS:
            assert r["files"][ext] == want["files"][ext], (chunk, ext)


def _vcf(path, records, n_samples=10, fmt="GT"):
    with open(path, "w") as f:
        f.write(HEADER + "".join("\tS%d" % j for j in range(n_samples)) + "\n")
        for chrom, pos, cells in records:
            f.write("%s\t%d\t.\tA\tC\t.\tPASS\t.\t%s\t%s\n" % (chrom, pos, fmt, "\t".join(cells)))


def refusal_cases(tmp_path):
    """the files of test_svd.py::test_refusals, and what each message holds"""
    gt = ["0/0", "0/1", "1/1"]
    cells = lambda i, n=10: [gt[(i * 7 + j * 3) % 3] for j in range(n)]      # noqa: E731
    ok = [("1", 100 + 10 * i, cells(i)) for i in range(12)]
    cases = [("and 9 samples", [(c, q, x[:9]) for c, q, x in ok], {"n_samples": 9}),
             ("9 markers kept", ok[:9] + [("X", 5, cells(1))], {}),
             ("Duplicated Marker at 1:140", ok[:5] + [ok[4]] + ok[5:], {}),
             ("Negative PL or Positive GL observed", [(c, q, ["30,0,%d" % (40 if (i, j) != (6, 3) else -40) for j in range(10)]) for i, (c, q, x) in enumerate(ok)], {"fmt": "PL"}),
             ("Cannot recognize GT, GL or PL key in FORMAT field", [(c, q, ["7"] * 10) for c, q, x in ok], {"fmt": "DP"}),
             ("fewer than two alleles", ok[:7] + [("1", 500, ["0/1"] * 6 + ["1"] + ["0/1"] * 3)] + ok[7:], {}),
             ("fewer than three values", [(c, q, ["0,30"] * 10) for c, q, x in ok], {"fmt": "PL"})]
    for k, (what, records, kw) in enumerate(cases):
        path = str(tmp_path / ("refusal%d.vcf" % k))
        _vcf(path, records, **kw)
        yield what, path


def check_refusals(reader, tmp_path):
    for what, path in refusal_cases(tmp_path):
        s0, s1 = api.Svd(host_eval=True), api.Svd(host_eval=True, reader=reader, chunk_bytes=4096)
        try:
            want = message(lambda: s0.read_vcf(path))
            got = message(lambda: s1.read_panel(path))
        finally:
            s0.close(); s1.close()
        print(got)
        assert what in want and got == want
        if "alleles" in what:
            assert "line 10" in got


def test_refusals_equal_the_serial_readers(tmp_path):
    check_refusals(2, tmp_path)


def test_sites_and_list_equal_the_serial_reader_on_the_filtered_file(tmp_path):
    check_sites_case(2, tmp_path)


def test_list_refusals(tmp_path):
    c = make_sites_case(str(tmp_path))
    other = write(str(tmp_path / "other.vcf"), c["head"].replace("H007", "H0x7").encode() + b"".join(c["line"](r).encode() for r in c["recs"] if r[0] == 2))
    s = api.Svd(host_eval=True, reader=2)
    try:
        m = message(lambda: s.read_panel([c["paths"][0], other]))
        assert "other.vcf" in m and "sample column 8" in m and "H0x7" in m
        # a duplicate across a file boundary: the second file begins with the first one's last record
        first = [r for r in c["recs"] if r[0] == 0]
        dup = write(str(tmp_path / "dup.vcf"), (c["head"] + c["line"](first[-1]) + "".join(c["line"](r) for r in c["recs"] if r[0] == 2)).encode())
        m = message(lambda: s.read_panel([c["paths"][0], dup]))
        assert m.startswith("Duplicated Marker at %s:%d" % (first[-1][1], first[-1][2])) and "line 3 of " + dup in m
        s.close()
        s = api.Svd(host_eval=True, reader=0)
        assert "serial reader" in message(lambda: s.read_panel([c["paths"][0], dup]))
    finally:
        s.close()


def test_cli_list_and_sites(tmp_path):
    c, want = check_sites_case(2, tmp_path)
    out = str(tmp_path / "cli")
    run = subprocess.run([CLI, "svd", "--RefVCFList", c["list"], "--Sites", c["sites"], "--Output", out, "--host_eval", "--chunk_bytes", "4096"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    err = run.stderr.decode()
    assert "host_loops reader" in err and "%d found in the panel, 4 not found" % c["n_found"] in err and "Success!" in err
    for ext in EXTS:
        assert read(out + ext) == want["files"][ext], ext
    run = subprocess.run([CLI, "svd", "--RefVCF", c["subset"], "--reader", "serial", "--Sites", c["sites"], "--Output", out + "2"], stderr=subprocess.PIPE, timeout=300)
    assert run.returncode != 0 and b"--reader serial" in run.stderr and not os.path.exists(out + "2.mu")
    run = subprocess.run([CLI, "svd", "--RefVCFList", c["list"], "--host_eval"], stderr=subprocess.PIPE, timeout=300)
    assert run.returncode != 0 and b"--RefVCFList needs --Output" in run.stderr


def test_bodies_under_sanitizers(tmp_path):
    """tests/vcf_check: the host-loop bodies over edge.vcf, p640x96 and texts cut short at the end of an exactly sized allocation; ASan + UBSan, a program of its own"""
    subprocess.check_call(["make", "-s", "-C", CHECK_DIR, "vcf_check"])
    plain = write(str(tmp_path / "p640x96.vcf"), text_of("p640x96"))
    run = subprocess.run([os.path.join(CHECK_DIR, "vcf_check"), str(tmp_path), vcf_of("edge"), plain], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert run.returncode == 0, (run.stdout.decode()[-2000:], run.stderr.decode()[-3000:])
    out = run.stdout.decode()
    print(out)
    assert out.count(", 0 differ") == 3 and "differ" not in out.replace(", 0 differ", "")
    assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr


# ---- GPU tier --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,chunk", CHUNKS)
def test_device_reader_equals_goldens_and_serial_reader(name, chunk, tmp_path):
    a = check_golden(name, chunk, 1, tmp_path)
    b = run_reader(vcf_of(name), 1, tmp_path, chunk=chunk, decompose=False)      # two runs: identical panels and stats
    strip = lambda st: {k: v for k, v in st.items() if k != "seconds"}      # noqa: E731
    assert same_panel(a["panel"], b["panel"]) and strip(a["stats"]) == strip(b["stats"])


SHAPES = [(40, 10, "GT", None), (64, 33, "PL", None), (30, 300, "PL", None), (12, 1100, "GT", None), (700, 16, "GT", 4096)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,fmt,chunk", SHAPES)
def test_device_genotype_kernel_shapes(M, N, fmt, chunk, tmp_path):
    """N = 300 GT:PL: a line crosses a 4 KiB tile; N = 1,100 GT: cells on every 16-byte and tile boundary; M = 700 at 4096-byte chunks: many chunks and carries"""
    G = np.random.default_rng(7 * M + N).integers(-1, 3, size=(M, N)).astype(np.int8)
    path = str(tmp_path / "p.vcf")
    synth.panel_vcf(path, G, fmt)
    want = run_reader(path, 0, tmp_path, decompose=False)
    got = run_reader(path, 1, tmp_path, chunk=chunk, decompose=False)
    assert same_panel(got["panel"], want["panel"])
    assert got["stats"]["host_lines"] == 0 and got["stats"]["kept"] == M
    if chunk:
        assert got["stats"]["chunks"] > 10


@pytest.mark.gpu
def test_device_bgzf_members(tmp_path):
    want = serial("p640x96")
    path = forms_of(text_of("p640x96"), tmp_path)["bgzf"]
    for chunk in (None, 4096):
        r = run_reader(path, 1, tmp_path, chunk=chunk, tag="bgzf")
        st = r["stats"]
        print(st)
        assert same_panel(r["panel"], want["panel"]) and st["members"] + st["members_host"] > 20 and st["members"] > 0 and st["host_lines"] == 0
        for ext in EXTS:
            assert r["files"][ext] == want["files"][ext], ext


@pytest.mark.gpu
def test_device_refusals_equal_the_serial_readers(tmp_path):
    check_refusals(1, tmp_path)


@pytest.mark.gpu
def test_device_sites_and_list(tmp_path):
    check_sites_case(1, tmp_path)


@pytest.mark.gpu
def test_cli_device_reader_and_device_decomposition(tmp_path):
    c = make_sites_case(str(tmp_path))
    a, b = str(tmp_path / "list"), str(tmp_path / "subset")
    run = subprocess.run([CLI, "svd", "--RefVCFList", c["list"], "--Sites", c["sites"], "--Output", a], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    assert b"device reader" in run.stderr and b"device kernels" in run.stderr and b"Success!" in run.stderr
    run = subprocess.run([CLI, "svd", "--RefVCF", c["subset"], "--Output", b], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0 and b"serial reader" in run.stderr, run.stderr.decode()[-2000:]
    for ext in EXTS:
        assert read(a + ext) == read(b + ext), ext
