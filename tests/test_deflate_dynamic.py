"""The BGZF compressor's dynamic mode (csrc/fq_deflate.h: fqd_member_dyn -- the parse of the fixed mode kept as tokens, code lengths made by the
wavefront, BTYPE = 10 per member where its exact cost is below the fixed code's) against zlib and against the fixed mode: every member sound and
never larger than the fixed encoding of its parse, the saving held to zlib's own on the same bytes, the code lengths complete, within their limit
and Huffman's where those fit, the writers and the command line with the mode switched on.  CPU tier: the bodies on the host-loop backend; GPU
tier: the kernels."""
import heapq
import math
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import oracle_binding as ob
import test_deflate_device as tdd
import test_sorted_bam as tsb
from fastquick_amd import api
from test_qc_consumer import QC_FILES, qc_bytes

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu")
BLOCK = 0xd000
Z_FIXED = getattr(zlib, "Z_FIXED", 4)


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "libfq_emu.so"])
    return api.load_library(os.path.join(EMU_DIR, "libfq_emu.so"))


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------------
def bam_like_skewed(n_rec=3000, seed=2):
    """aligned BAM records as the writer packs them: both nibbles of a SEQ byte in {1, 2, 4, 8} (A C G T), qualities clip(38 - geometric(0.25), 2, 41)"""
    rng = np.random.default_rng(seed)
    nib = np.array([1, 2, 4, 8], dtype=np.uint8)
    out = []
    for i in range(n_rec):
        seq = (nib[rng.integers(0, 4, 75)] << 4 | nib[rng.integers(0, 4, 75)]).astype(np.uint8).tobytes()
        qual = np.clip(38 - rng.geometric(0.25, 150), 2, 41).astype(np.uint8).tobytes()
        out.append(struct.pack("<iiBBHHHiiii", 3, 1000 + i, 11, 60, 4681, 1, 99, 150, 3, 1300 + i, 450) + b"r%09d\0" % i + seq + qual + b"XTAUNMC\0SMC%AMC%X0C\1X1C\0XMC\0XOC\0XGC\0MDZ150\0")
    return b"".join(out)


def no_four_byte_repeat(n=BLOCK, seed=3):
    """n bytes in which no window of four bytes occurs twice: the parse finds no match"""
    rng = np.random.default_rng(seed)
    draw = rng.integers(0, 256, 2 * n, dtype=np.uint8).tolist()
    out, seen, k = bytearray(), set(), 0
    while len(out) < n:
        c = draw[k]; k += 1
        w = bytes(out[-3:]) + bytes([c])
        if len(w) == 4 and w in seen:
            continue
        seen.add(w)
        out.append(c)
    return bytes(out)


_CASES = {}


def new_cases():
    if not _CASES:
        rng = np.random.default_rng(5)
        two = np.array([65, 200], dtype=np.uint8)
        _CASES.update({
            "AAA": b"AAA",                                             # two literal symbols (A and the end of block), no match
            "one_byte_repeated": b"Q" * BLOCK,                         # one distance, one length: the two-codes rule
            "two_values": two[rng.integers(0, 2, BLOCK)].tobytes(),
            "bam_like_skewed": bam_like_skewed(),
            "no_four_byte_repeat": no_four_byte_repeat(),
            "size_0": b"", "size_1": b"\x07",
            "size_block_minus_1": rng.integers(0, 7, BLOCK - 1, dtype=np.uint8).tobytes(),
            "size_block_plus_1": rng.integers(0, 7, BLOCK + 1, dtype=np.uint8).tobytes(),
        })
    return _CASES


_ALL = {}


def all_cases():
    if not _ALL:
        _ALL.update(tdd.cases())
        _ALL.update(new_cases())
    return _ALL


def split_members(blob):
    out, at = [], 0
    while at < len(blob):
        bsize = struct.unpack_from("<H", blob, at + 16)[0] + 1
        out.append(blob[at:at + bsize])
        at += bsize
    return out


def btype(member):
    return member[18] >> 1 & 3


def host_inflate(lib, member, isize):
    """the raw DEFLATE payload of a member through the host decoder (fq_inflate_raw)"""
    C = api.C
    src = member[18:-8]
    keep, out = C.create_string_buffer(src, max(1, len(src))), C.create_string_buffer(max(1, isize))
    rc = lib.fq_inflate_raw(C.cast(keep, C.c_void_p), len(src), C.cast(out, C.c_void_p), isize)
    assert rc == 0, "fq_inflate_raw refused a member of %d bytes: %d" % (isize, rc)
    return out.raw[:isize]


# ---- 1 - 3. soundness, block type, never larger ---------------------------------------------------------------------------------------------------
def check_soundness(lib, **dev):
    for name, data in all_cases().items():
        z, _ = api.bgzf_deflate_device(data, lib=lib, mode="dynamic", **dev)
        back, n = tdd.members(z)
        assert back == data, name
        assert n == (len(data) + BLOCK - 1) // BLOCK, name
        at = 0
        for m in split_members(z):
            isz = struct.unpack("<I", m[-4:])[0]
            assert host_inflate(lib, m, isz) == data[at:at + isz], name
            at += isz


def check_block_types(lib, **dev):
    types = {}
    for name in ("empty", "nine_bit_literals", "bam_like_skewed", "one_byte", "AAA"):
        data = all_cases()[name]
        z, _ = api.bgzf_deflate_device(data, lib=lib, mode="dynamic", **dev)
        ms = split_members(z)
        types[name] = [btype(m) for m in ms]
        full = [btype(m) for m, k in zip(ms, range(len(ms))) if len(data) - k * BLOCK >= BLOCK]
        if name in ("nine_bit_literals", "bam_like_skewed"):
            assert full and all(t == 2 for t in full), (name, types[name])
    # (the empty input is no member at all: there is no byte 18 to read; the smallest members, where tables cannot pay, stay BTYPE = 01)
    assert types["empty"] == [] and types["one_byte"] == [1] and types["AAA"] == [1], types
    return types


def check_never_larger(lib, per_member, **dev):
    for name, data in all_cases().items():
        old, _ = api.bgzf_deflate_device(data, lib=lib, **dev)
        fixed, _ = api.bgzf_deflate_device(data, lib=lib, mode="fixed", mode_entry=True, **dev)
        dyn, _ = api.bgzf_deflate_device(data, lib=lib, mode="dynamic", **dev)
        if per_member:      # the host-loop tier: the parse is deterministic
            assert fixed == old, name
            mf, md = split_members(fixed), split_members(dyn)
            assert len(mf) == len(md) and all(len(d) <= len(f) for f, d in zip(mf, md)), (name, [len(m) for m in mf], [len(m) for m in md])
        else:               # the hash-slot race is the hardware's to resolve: totals
            assert len(dyn) <= len(fixed), (name, len(fixed), len(dyn))


def test_dynamic_members_are_sound_on_the_host_loop_backend(emu_lib):
    check_soundness(emu_lib)


def test_block_type_is_chosen_per_member_on_the_host_loop_backend(emu_lib):
    check_block_types(emu_lib)


def test_dynamic_is_never_larger_and_fixed_is_unchanged_on_the_host_loop_backend(emu_lib):
    check_never_larger(emu_lib, True)


# ---- 4. the saving, held to zlib's on the same bytes ---------------------------------------------------------------------------------------------
def zlib_blocks(data, level, strategy):
    total = 0
    for lo in range(0, len(data), BLOCK):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += len(c.compress(data[lo:lo + BLOCK]) + c.flush()) + 26
    return total


def check_saving(lib, **dev):
    data = all_cases()["bam_like_skewed"]
    r_z = zlib_blocks(data, 1, zlib.Z_DEFAULT_STRATEGY) / zlib_blocks(data, 1, Z_FIXED)
    fixed, _ = api.bgzf_deflate_device(data, lib=lib, **dev)
    dyn, _ = api.bgzf_deflate_device(data, lib=lib, mode="dynamic", **dev)
    z6 = zlib_blocks(data, 6, zlib.Z_DEFAULT_STRATEGY)
    r = len(dyn) / len(fixed)
    print("BAM-like records, %d bytes: zlib-1 dynamic / fixed = %.4f ; device dynamic / fixed = %.4f (%d / %d bytes) ; against zlib-6 (%d bytes): fixed %.4f, dynamic %.4f"
          % (len(data), r_z, r, len(dyn), len(fixed), z6, len(fixed) / z6, len(dyn) / z6))
    assert r <= 1 - 0.5 * (1 - r_z), (r, r_z)


def test_saving_on_bam_like_records_on_the_host_loop_backend(emu_lib):
    check_saving(emu_lib)


# ---- 5. the code lengths alone --------------------------------------------------------------------------------------------------------------------
def huffman(freq):
    """(cost, deepest code) of a Huffman code over the used symbols, by heapq; ties go to the shallower subtree"""
    heap = [(int(f), 0, s) for s, f in enumerate(freq) if f]
    if len(heap) < 2:
        return None
    heapq.heapify(heap)
    cost, tick = 0, len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, tick))
        tick += 1
    return cost, heap[0][1]


def package_merge(freq, limit):
    """the cost of an optimal code of at most `limit` bits over the used symbols (Larmore / Hirschberg)"""
    leaves = sorted((int(f), (s,)) for s, f in enumerate(freq) if f)
    n = len(leaves)
    row = leaves
    for _ in range(limit - 1):
        packs = [(row[k][0] + row[k + 1][0], row[k][1] + row[k + 1][1]) for k in range(0, len(row) - 1, 2)]
        row = sorted(leaves + packs, key=lambda t: t[0])
    lens = {}
    for _, syms in row[:2 * n - 2]:
        for s in syms:
            lens[s] = lens.get(s, 0) + 1
    return sum(int(freq[s]) * l for s, l in lens.items())


def length_vectors():
    rng = np.random.default_rng(11)
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    out = []
    for n, limit in ((286, 15), (30, 15), (19, 7)):
        out.append(("all_zero_%d" % n, [0] * n, limit))
        one = [0] * n; one[n // 3] = 9
        out.append(("one_used_%d" % n, one, limit))
        first = [0] * n; first[0] = 4
        out.append(("only_symbol_0_%d" % n, first, limit))
        second = [0] * n; second[1] = 4
        out.append(("only_symbol_1_%d" % n, second, limit))
        two = [0] * n; two[2] = 1; two[n - 1] = 1000
        out.append(("two_used_%d" % n, two, limit))
        out.append(("all_equal_%d" % n, [3] * n, limit))
    out.append(("powers_of_two_15", [1 << k for k in range(15)] + [0] * 15, 15))
    out.append(("powers_of_two_7", [1 << k for k in range(7)] + [0] * 12, 7))
    out.append(("powers_of_two_20_beyond_the_limit", [1 << k for k in range(20)] + [0] * 10, 15))
    out.append(("fibonacci_19_limit_7", fib[:19], 7))
    out.append(("fibonacci_24_limit_15", fib[:24] + [0] * 6, 15))
    for k in range(20):
        n, limit = ((286, 15), (30, 15), (19, 7))[k % 3]
        f = rng.integers(0, 1 << int(rng.integers(1, 17)), n) * (rng.random(n) < rng.choice([0.1, 0.4, 0.9]))
        out.append(("random_%d" % k, [int(v) for v in f], limit))
    return out


def check_lengths(lib, **dev):
    report = []
    for name, freq, limit in length_vectors():
        lens = [int(v) for v in api.huffman_lengths_device(freq, limit, lib=lib, **dev)]
        used = [s for s, f in enumerate(freq) if f]
        coded = [s for s, l in enumerate(lens) if l]
        assert all(1 <= lens[s] <= limit for s in used), name
        if len(used) >= 2:
            assert coded == used, name
        else:       # the two-codes rule: the missing codes go to symbols of frequency 0, one bit each
            assert len(coded) == 2 and set(used) <= set(coded) and all(lens[s] == 1 for s in coded), (name, coded)
        assert sum(2 ** (limit - lens[s]) for s in coded) == 2 ** limit, "%s: the code is not complete" % name
        h = huffman(freq)
        if h is None:
            continue
        cost = sum(int(freq[s]) * lens[s] for s in used)
        if h[1] <= limit:
            assert cost == h[0], (name, cost, h)
        else:
            flat = sum(int(freq[s]) for s in used) * max(1, math.ceil(math.log2(len(used))))
            best = package_merge(freq, limit)
            assert best <= cost <= flat, (name, best, cost, flat)
            report.append((name, limit, len(used), h[0], best, cost))
            print("code lengths beyond the limit: %-36s limit %2d, %3d used: Huffman %d bits (depth %d), package-merge %d, the repair %d (+%.3f %%)"
                  % (name, limit, len(used), h[0], h[1], best, cost, 100.0 * (cost - best) / best))
    assert len(report) >= 3, "the vectors must reach the limiter"
    return report


def test_code_lengths_on_the_host_loop_backend(emu_lib):
    check_lengths(emu_lib)


def test_code_length_entry_refuses_what_it_cannot_code(emu_lib):
    for freq, limit in (([1], 15), ([1] * 289, 15), ([1] * 19, 4), ([1] * 19, 0), ([1] * 19, 16), ([1 << 31, 1 << 31], 15)):
        with pytest.raises(api.FastquickError):
            api.huffman_lengths_device(freq, limit, lib=emu_lib)


# ---- 6. the writers ---------------------------------------------------------------------------------------------------------------------------------
def write_bam(g, lib, path, sorted_file, deflate, se=False, **dev):
    """the case's reads through a context with the writer attached, batch by batch: the writer's (deflate mode, fixed members, dynamic members) before the close"""
    names, seq, qual, lens = ob.read_fastq_pair(g["fq1"], g["fq2"])
    if se:
        names, seq, qual, lens = list(names), seq[:1], qual[:1], lens[:1]
    ix = api.Index(g["prefix"], lib=lib, **dev)
    al = api.Aligner(ix, api.default_opts(lib, trim_qual=g["trim_qual"], single_end=1 if se else 0), max_pairs=max(16, g["batch"]))
    W = api.BamWriter(ix, os.path.join(g["dir"], "genome.fai"), path, sorted=sorted_file, deflate=deflate)
    W.attach(al)
    for lo in range(0, seq.shape[1], g["batch"]):
        hi = min(seq.shape[1], lo + g["batch"])
        al.align(seq[:, lo:hi], qual[:, lo:hi], lens[:, lo:hi], names[lo:hi])
        W.add(al)
    st = W.deflate_stats()
    W.close()
    al.close(); ix.close()
    return st


def file_types(path):
    return [btype(m) for m in split_members(open(path, "rb").read())]


def check_writers(g, lib, tmp, se, **dev):
    p = {k: os.path.join(tmp, k + ".bam") for k in ("uf", "ud", "sf", "sd")}
    st = {k: write_bam(g, lib, p[k], k[0] == "s", "dynamic" if k[1] == "d" else "fixed", se=se, **dev) for k in p}
    assert st["uf"] == ("fixed", 0, 0) and st["ud"][0] == "dynamic" and st["ud"][2] > 0
    UF, UD, SF, SD = (tsb.load(p[k]) for k in ("uf", "ud", "sf", "sd"))
    assert len(UF.records) > 0 and UD.payload == UF.payload and SD.payload == SF.payload
    # the device's members of the dynamic files: as many as the writer counted, and the files smaller for them
    assert file_types(p["ud"]).count(2) >= st["ud"][2] > 0 and 2 in file_types(p["sd"])
    assert os.path.getsize(p["ud"]) < os.path.getsize(p["uf"]) and os.path.getsize(p["sd"]) < os.path.getsize(p["sf"])
    tsb.check_sorted_against_unsorted(p["sd"], UF)
    tsb.check_index(SD, 20)      # (the index through the dynamic file's own virtual offsets: every region's records against the brute-force answer, which is the fixed file's)
    tsb.check_index(SF, 20)


WRITER_CASES = [("qc", False)] + [(t, True) for t in tsb.SE_CONSUMER_TAGS[:1]]


@pytest.mark.parametrize("tag,se", WRITER_CASES)
def test_writers_in_dynamic_mode_on_the_host_loop_backend(tag, se, golden_cases, emu_lib, tmp_path):
    check_writers(golden_cases[tag], emu_lib, str(tmp_path), se)


def test_mode_is_set_before_records_and_the_call_wins_over_the_environment(golden_cases, emu_lib, tmp_path, monkeypatch):
    g = golden_cases["qc"]
    ix = api.Index(g["prefix"], lib=emu_lib)
    fai = os.path.join(g["dir"], "genome.fai")
    monkeypatch.delenv("FASTQUICK_BAM_DEFLATE", raising=False)
    w = api.BamWriter(ix, fai, str(tmp_path / "a.bam"))
    assert w.deflate_stats()[0] == "fixed"
    for bad in (7, -1, 2):
        with pytest.raises(api.FastquickError):
            w.set_deflate(bad)
    w.set_deflate("dynamic")
    assert w.deflate_stats()[0] == "dynamic"
    w.set_deflate(0)
    w.write_records(b"")
    with pytest.raises(api.FastquickError):      # records have been taken
        w.set_deflate("dynamic")
    assert w.deflate_stats()[0] == "fixed"
    w.close()
    monkeypatch.setenv("FASTQUICK_BAM_DEFLATE", "dynamic")
    w = api.BamWriter(ix, fai, str(tmp_path / "b.bam"))
    assert w.deflate_stats()[0] == "dynamic"
    w.close()
    w = api.BamWriter(ix, fai, str(tmp_path / "c.bam"), deflate="fixed")
    assert w.deflate_stats()[0] == "fixed"
    w.close()
    monkeypatch.setenv("FASTQUICK_BAM_DEFLATE", "fixed")
    w = api.BamWriter(ix, fai, str(tmp_path / "d.bam"), sorted=True)
    assert w.deflate_stats()[0] == "fixed"
    w.close()
    ix.close()
    # the variable selects what the device writes: the whole feeding of the sorted-file tests under it
    monkeypatch.setenv("FASTQUICK_BAM_DEFLATE", "dynamic")
    path, _, _ = tsb.feed(g, emu_lib, str(tmp_path / "env"), g["batch"], True)
    assert 2 in file_types(path["S"])
    monkeypatch.setenv("FASTQUICK_BAM_DEFLATE", "fixed")
    path_f, _, _ = tsb.feed(g, emu_lib, str(tmp_path / "envf"), g["batch"], True)
    assert tsb.load(path_f["S"]).payload == tsb.load(path["S"]).payload and os.path.getsize(path["S"]) < os.path.getsize(path_f["S"])


# ---- 7. the command line --------------------------------------------------------------------------------------------------------------------------
def qc_files(out):
    return {f: qc_bytes(out + "." + f).replace(out.encode(), b"OUT") for f in QC_FILES}


def check_command_line(run, out, gpu):
    """run(tag, *extra, ok=True, bam_in=None) -> the finished process; out(tag) -> the run's prefix"""
    runs = {tag: run(tag, *extra) for tag, extra in (("f", []), ("d", ["--bam_deflate", "dynamic"]), ("sf", ["--sorted_bam"]), ("sd", ["--sorted_bam", "--bam_deflate", "dynamic"]))}
    F, D = tsb.load(out("f") + ".bam"), tsb.load(out("d") + ".bam")
    SF, SD = tsb.load(out("sf") + ".sorted.bam"), tsb.load(out("sd") + ".sorted.bam")
    assert len(F.records) > 0 and D.payload == F.payload and SD.payload == SF.payload
    assert os.path.getsize(out("d") + ".bam") < os.path.getsize(out("f") + ".bam") and os.path.getsize(out("sd") + ".sorted.bam") < os.path.getsize(out("sf") + ".sorted.bam")
    tsb.check_index(SD, 20)
    want = qc_files(out("f"))
    assert len(want) == 13
    for tag in ("d", "sf", "sd"):
        assert qc_files(out(tag)) == want, tag
    for tag in ("f", "sf"):
        assert b"NOTICE - BAM writer: deflate mode fixed" in runs[tag].stderr
    for tag, path in (("d", out("d") + ".bam"), ("sd", out("sd") + ".sorted.bam")):
        m = re.search(rb"NOTICE - BAM writer: deflate mode dynamic.*: (\d+) of the device's members took dynamic Huffman tables, (\d+) the fixed code", runs[tag].stderr)
        assert m, runs[tag].stderr.decode(errors="replace")[-2000:]
        n_dyn, n_fix = int(m.group(1)), int(m.group(2))
        assert n_dyn > 0 and file_types(path).count(2) >= n_dyn and n_dyn + n_fix <= len(file_types(path)) - 1
    # the device front end's own decoder over these members: O.bam of either mode as the input of a run gives the same text and the same files
    sam = {tag: run("b" + tag, "--sam_out", bam_in=out(tag) + ".bam") for tag in ("f", "d")}
    assert sam["f"].stdout == sam["d"].stdout and any(ln and not ln.startswith(b"@") for ln in sam["d"].stdout.split(b"\n"))
    named = lambda tag: {f: v.replace(os.path.basename(out(tag)).encode() + b".bam", b"IN.bam") for f, v in qc_files(out("b" + tag)).items()}      # (FASTQ.csv names the input)
    assert named("d") == named("f")
    if gpu:
        for tag in ("f", "d"):
            m = re.search(rb"front end on the device: \d+ pairs, (\d+) BGZF members \((\d+) left to the host's decoder\)", sam[tag].stderr)
            assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0, sam[tag].stderr.decode(errors="replace")[-2000:]
    bad = run("x", "--bam_deflate", "dynamic", "--sam_out", ok=False)
    assert bad.returncode != 0 and b"--bam_deflate" in bad.stderr and b"--sam_out" in bad.stderr and not bad.stdout
    bad = run("y", "--bam_deflate", "best", ok=False)
    assert bad.returncode != 0 and b"--bam_deflate takes fixed or dynamic" in bad.stderr
    assert not [f for f in os.listdir(os.path.dirname(out("x"))) if os.path.basename(f).startswith(("x.", "y."))]


def test_command_line_bam_deflate(golden_cases, emu_cli, tmp_path):
    g = golden_cases["qc"]
    tsb.write_param(g)
    out = lambda tag: str(tmp_path / tag)

    def run(tag, *extra, ok=True, bam_in=None):
        inputs = ["--bam_in", bam_in] if bam_in else ["--fastq_1", g["fq1"], "--fastq_2", g["fq2"]]
        cmd = [emu_cli, "align", "--index_prefix", g["prefix"][:-len(".FASTQuick.fa")], "--out_prefix", out(tag), "--batch_pairs", str(g["batch"]), "--chunk_pairs", str(g["batch"]),
               "--q", str(g["trim_qual"]), "--read_len", str(g["qc_read_len"])] + inputs + list(extra)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert (r.returncode == 0) == ok, r.stderr.decode(errors="replace")[-3000:]
        return r

    check_command_line(run, out, False)


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_dynamic_members_are_sound_on_the_gpu():
    check_soundness(api.load_library(), device=0)


@pytest.mark.gpu
def test_block_type_is_chosen_per_member_on_the_gpu():
    check_block_types(api.load_library(), device=0)


@pytest.mark.gpu
def test_dynamic_is_never_larger_on_the_gpu():
    check_never_larger(api.load_library(), False, device=0)


@pytest.mark.gpu
def test_saving_on_bam_like_records_on_the_gpu():
    check_saving(api.load_library(), device=0)


@pytest.mark.gpu
def test_code_lengths_on_the_gpu():
    check_lengths(api.load_library(), device=0)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,se", WRITER_CASES)
def test_writers_in_dynamic_mode_on_the_gpu(tag, se, golden_cases, tmp_path):
    check_writers(golden_cases[tag], api.load_library(), str(tmp_path), se, device=0)


@pytest.mark.gpu
def test_larger_input_on_the_gpu_and_both_kernels_rates():
    lib = api.load_library()
    data = all_cases()["bam_like_skewed"] * 200
    for mode in ("fixed", "dynamic"):
        z, ms = api.bgzf_deflate_device(data, lib=lib, mode=mode, mode_entry=True)
        back, n = tdd.members(z)
        assert back == data and n == (len(data) + BLOCK - 1) // BLOCK
        print("device BGZF, %s: %.1f MB -> %.1f MB in %.2f ms = %.1f GB/s" % (mode, len(data) / 1e6, len(z) / 1e6, ms, len(data) / ms / 1e6))


@pytest.mark.gpu
def test_command_line_bam_deflate_on_the_gpu(tmp_path):
    """the real FASTQuick_amd align, every run a process of its own under a time limit, on the seeded synthetic input of the sorted-file test"""
    case = tsb.make_synth_fastq(str(tmp_path))
    out = case["out"]

    def run(tag, *extra, ok=True, bam_in=None):
        inputs = ["--bam_in", bam_in] if bam_in else ["--fastq_1", case["fq"][0], "--fastq_2", case["fq"][1]]
        cmd = [tsb.CLI_GPU, "align", "--index_prefix", case["prefix"], "--out_prefix", out(tag), "--read_len", "151", "--chunk_pairs", "8192", "--batch_pairs", "4096"] + inputs + list(extra)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=tsb.GPU_STEP_SEC)
        assert (r.returncode == 0) == ok, r.stderr.decode(errors="replace")[-3000:]
        return r

    check_command_line(run, out, True)
