"""The coordinate-sorted BAM writer and its index (fq_bam_create_sorted; csrc/fq_sort.h): what the pipeline's `samtools sort` / `samtools index` steps make of O.bam.
The sorted file is DEFINED as the stable sort, by (reference id as unsigned, position, strand), of the records the unsorted writer of the same library writes; the
key, reg2bin / reg2bins and the .bai reader below are restated here from that definition and the SAM specification (5.2, 5.3) -- the library is not asked for them.
CPU tier: the host-loop library (the launchers of fq_sort.h as loops over the kernels' bodies, the attached path included); GPU tier: the kernels."""
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import golden_util
import oracle_binding as ob
from fastquick_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")
CLI_GPU = os.path.join(ROOT, "fastquick_amd", "bin", "FASTQuick_amd")
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
HD_LINE = "@HD\tVN:1.6\tSO:coordinate\n"
GPU_STEP_SEC = 120      # every GPU step that is a process of its own ends after this long


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "libfq_emu.so"])
    return api.load_library(os.path.join(EMU_DIR, "libfq_emu.so"))


# ---- 1. the sort entry against numpy's stable argsort -------------------------------------------------------------------------
SORT_SIZES = [0, 1, 2, 63, 64, 65] + [v for k in range(8, 15) for v in (2 ** k - 1, 2 ** k, 2 ** k + 1)]
KEY_BITS = [1, 8, 9, 34, 64]
PATTERNS = ["equal", "two_alternating", "ascending", "descending", "top_digit", "lowest_bit", "random"]


def key_pattern(name, n, key_bits, rng):
    top = 8 * ((key_bits - 1) // 8)      # the first bit of the key's top digit
    i = np.arange(n, dtype=np.uint64)
    if name == "equal":
        k = np.full(n, 0x5a5a5a5a5a5a5a5a, np.uint64)
    elif name == "two_alternating":
        k = np.where(i % np.uint64(2) == 0, np.uint64(0xfedcba9876543210), np.uint64(0x0123456789abcdef))
    elif name == "ascending":
        k = i
    elif name == "descending":
        k = i[::-1].copy()
    elif name == "top_digit":
        k = rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(top)
    elif name == "lowest_bit":
        k = np.uint64(0x1234567800) | rng.integers(0, 2, n, dtype=np.uint64)
    else:
        k = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    return k & np.uint64((1 << key_bits) - 1)


def check_sort_sizes(lib, sizes, **dev):
    rng = np.random.default_rng(20261018)
    for n in sizes:
        for key_bits in KEY_BITS:
            for name in PATTERNS:
                keys = key_pattern(name, n, key_bits, rng)
                perm, _ = api.sort_keys_device(keys, key_bits, lib=lib, **dev)
                want = np.argsort(keys, kind="stable").astype(np.uint32)
                assert perm.shape == want.shape and (perm == want).all(), "n = %d, %d key bits, %s" % (n, key_bits, name)


def test_sort_is_the_stable_permutation_on_the_host_loop_backend(emu_lib):
    check_sort_sizes(emu_lib, SORT_SIZES)


def test_sort_entry_refuses_what_it_cannot_sort(emu_lib):
    k = np.zeros(4, np.uint64)
    for bits in (0, 65, -1):
        with pytest.raises(api.FastquickError):
            api.sort_keys_device(k, bits, lib=emu_lib)


# ---- the BAM file and its index, read from the specification -----------------------------------------------------------------
class BamFile:
    """path's BGZF members, what they inflate to, header and records as raw bytes; payload offset <-> virtual offset"""

    def __init__(self, path):
        blob = open(path, "rb").read()
        self.member_off, self.member_start, parts, at, total = [], [], [], 0, 0
        while at < len(blob):
            assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12:at + 16] == b"BC\x02\x00", "not a BGZF block at %d" % at
            bsize = struct.unpack_from("<H", blob, at + 16)[0] + 1
            data = zlib.decompress(blob[at + 18:at + bsize - 8], -15)
            crc, isz = struct.unpack_from("<II", blob, at + bsize - 8)
            assert zlib.crc32(data) == crc and len(data) == isz and isz <= 65536
            self.member_off.append(at); self.member_start.append(total)
            parts.append(data); total += len(data)
            at += bsize
        assert at == len(blob) and len(parts) >= 2 and blob[-28:] == EOF_BLOCK, "check_bgzf: whole members, the end-of-file block last"
        self.eof_voff = self.member_off[-1] << 16
        p = self.payload = b"".join(parts)
        assert p[:4] == b"BAM\x01"
        l_text = struct.unpack_from("<i", p, 4)[0]
        self.text = p[8:8 + l_text].decode()
        at = 8 + l_text
        n_ref = struct.unpack_from("<i", p, at)[0]
        at += 4
        self.refs = []
        for _ in range(n_ref):
            l_name = struct.unpack_from("<i", p, at)[0]
            self.refs.append((p[at + 4:at + 4 + l_name - 1].decode(), struct.unpack_from("<i", p, at + 4 + l_name)[0]))
            at += 8 + l_name
        self.rec_at, self.records = [], []
        while at < len(p):
            n = struct.unpack_from("<i", p, at)[0] + 4
            assert n >= 36 and at + n <= len(p)
            self.rec_at.append(at); self.records.append(p[at:at + n])
            at += n
        self.at_of = {a: i for i, a in enumerate(self.rec_at)}
        self.pos_bits = (max([ln for _, ln in self.refs] + [0]) + 1).bit_length()

    def payload_of(self, voff):
        m = np.searchsorted(self.member_off, voff >> 16, side="right") - 1
        assert self.member_off[m] == voff >> 16, "a virtual offset must name the start of a member"
        return self.member_start[m] + (voff & 0xffff)

    def voff_of(self, at):
        m = int(np.searchsorted(self.member_start, at, side="right")) - 1
        while m + 1 < len(self.member_start) and self.member_start[m + 1] == at:      # (a record at a member's end belongs to the next member's start)
            m += 1
        return self.member_off[m] << 16 | (at - self.member_start[m])


def fields(rec):
    """refID, pos, flag and the end of the alignment: pos + the reference length of M D N = X; pos + 1 when that is 0 or flag 4 is set"""
    rid, pos, l_name, _mapq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    rlen = sum(c >> 4 for c in struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name) if (c & 15) in (0, 2, 3, 7, 8))
    return rid, pos, flag, (pos + 1 if (flag & 4) or rlen == 0 else pos + rlen)


def sort_key(rec, n_ref, pos_bits):
    rid, pos, flag, _ = fields(rec)
    tid = n_ref if rid < 0 else rid
    return tid << (pos_bits + 1) | (0 if pos < -1 else pos + 1) << 1 | (flag >> 4 & 1)


def split_records(raw):
    out, at = [], 0
    while at < len(raw):
        n = struct.unpack_from("<i", raw, at)[0] + 4
        out.append(raw[at:at + n])
        at += n
    return out


def check_sorted_against_unsorted(sorted_path, unsorted):
    s = BamFile(sorted_path)
    assert s.text == HD_LINE + unsorted.text and s.refs == unsorted.refs
    n_ref, pos_bits = len(unsorted.refs), unsorted.pos_bits
    want = sorted(unsorted.records, key=lambda r: sort_key(r, n_ref, pos_bits))      # (Python's sort is stable)
    assert len(s.records) == len(want)
    assert s.records == want, "first difference at record %d" % next(i for i, (a, b) in enumerate(zip(s.records, want)) if a != b)
    return s


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins += range(first + (beg >> shift), first + (end >> shift) + 1)
    return bins


class Bai:
    def __init__(self, path):
        d = open(path, "rb").read()
        assert d[:4] == b"BAI\x01"
        n_ref, at = struct.unpack_from("<i", d, 4)[0], 8
        self.refs = []
        for _ in range(n_ref):
            n_bin = struct.unpack_from("<i", d, at)[0]
            at += 4
            bins, pseudo = {}, None
            for _ in range(n_bin):
                b, n_chunk = struct.unpack_from("<Ii", d, at)
                at += 8
                chunks = [struct.unpack_from("<QQ", d, at + 16 * k) for k in range(n_chunk)]
                at += 16 * n_chunk
                if b == 37450:
                    assert n_chunk == 2 and pseudo is None
                    pseudo = chunks
                else:
                    assert b not in bins and b < 37449 and n_chunk > 0
                    bins[b] = chunks
            n_intv = struct.unpack_from("<i", d, at)[0]
            at += 4
            lin = list(struct.unpack_from("<%dQ" % n_intv, d, at))
            at += 8 * n_intv
            self.refs.append((bins, lin, pseudo))
        self.n_no_coor = struct.unpack_from("<Q", d, at)[0]
        assert at + 8 == len(d)


def interval(rec):
    rid, pos, flag, end = fields(rec)
    beg = max(pos, 0)
    return rid, beg, max(end, beg + 1), flag


def query(bam, bai, tid, beg, end):
    """the records of [beg, end) on tid through the index: reg2bins, the linear index's cut, seek to a chunk's start, decode to its end"""
    bins, lin, _ = bai.refs[tid]
    if (beg >> 14) >= len(lin):
        return []                      # no record reaches this window or a later one
    min_off = lin[beg >> 14]
    hits = set()
    for b in reg2bins(beg, end):
        for c0, c1 in bins.get(b, ()):
            if c1 <= min_off:
                continue
            at, stop = bam.payload_of(c0), bam.payload_of(c1) if c1 != bam.eof_voff else len(bam.payload)
            while at < stop:
                i = bam.at_of[at]          # (KeyError: a chunk that does not begin at a record)
                rid, rbeg, rend, _ = interval(bam.records[i])
                if rid == tid and rbeg < end and rend > beg:
                    hits.add(i)
                at += len(bam.records[i])
            assert at == stop, "a chunk must end where a record ends"
    return sorted(hits)


def regions_of(bam, n, seed):
    rng = np.random.default_rng(seed)
    iv = [interval(r) for r in bam.records]
    placed = [(rid, b, e) for rid, b, e, _ in iv if rid >= 0]
    out = []
    for tid, (_, ln) in enumerate(bam.refs):
        out.append((tid, 0, max(ln, 1)))                                  # whole chromosomes
        mine = [(b, e) for rid, b, e in placed if rid == tid]
        top = max([e for _, e in mine] + [0])
        out.append((tid, top + 5, top + 5 + 20000))                       # an empty stretch behind the last record (or a whole empty chromosome)
    for k in rng.permutation(len(placed))[:12]:                               # around marker positions, and the 16,384 boundaries next to them
        tid, b, e = placed[k]
        out += [(tid, max(b - 3, 0), b + 1), (tid, b, e), (tid, e - 1, e + 40)]
        w = (b >> 14) << 14
        for edge in (w, w + 16384):
            if edge > 0:
                out += [(tid, edge - 1, edge), (tid, edge, edge + 1), (tid, max(edge - 200, 0), edge + 200)]
    while len(out) < n and bam.refs:
        tid = int(rng.integers(0, len(bam.refs)))
        a = int(rng.integers(0, max(bam.refs[tid][1], 2)))
        out.append((tid, a, a + int(rng.integers(1, 40000))))
    return out[:max(n, 2 * len(bam.refs))]


def check_index(sorted_bam, n_regions=50, seed=1):
    bam = sorted_bam
    bai = Bai(bam_path_of[id(bam)] + ".bai")
    assert len(bai.refs) == len(bam.refs)
    iv = [interval(r) for r in bam.records]
    assert bai.n_no_coor == sum(1 for rid, _, _, _ in iv if rid < 0)
    for tid, (bins, lin, pseudo) in enumerate(bai.refs):
        mine = [i for i, (rid, _, _, _) in enumerate(iv) if rid == tid]
        for b, chunks in bins.items():
            assert all(c0 < c1 for c0, c1 in chunks) and all(chunks[k][1] <= chunks[k + 1][0] for k in range(len(chunks) - 1)), "chunks of bin %d ascend and are disjoint" % b
        if not mine:
            assert pseudo is None and not bins and not lin
            continue
        assert pseudo is not None
        assert pseudo[1] == (sum(1 for i in mine if not iv[i][3] & 4), sum(1 for i in mine if iv[i][3] & 4)), "mapped / unmapped counts of the pseudo-bin"
        last_end = bam.rec_at[mine[-1]] + len(bam.records[mine[-1]])
        assert pseudo[0] == (bam.voff_of(bam.rec_at[mine[0]]), bam.voff_of(last_end) if last_end < len(bam.payload) else bam.eof_voff)
        # every record lies in the bin reg2bin names, inside one of its chunks; the linear index per window from its definition
        want_lin = {}
        for i in mine:
            _, b, e, _ = iv[i]
            v = bam.voff_of(bam.rec_at[i])
            assert any(c0 <= v < c1 for c0, c1 in bins.get(reg2bin(b, e), ())), "record %d is not in a chunk of its bin" % i
            for w in range(b >> 14, ((e - 1) >> 14) + 1):
                want_lin[w] = min(want_lin.get(w, v), v)
        assert len(lin) == max(want_lin) + 1
        for w in range(len(lin) - 1, -1, -1):
            assert lin[w] == (want_lin[w] if w in want_lin else lin[w + 1]), "linear index, window %d" % w
    regions = regions_of(bam, n_regions, seed)
    assert len(regions) >= n_regions
    n_hits = 0
    for tid, beg, end in regions:
        brute = [i for i, (rid, b, e, _) in enumerate(iv) if rid == tid and b < end and e > beg]
        assert query(bam, bai, tid, beg, end) == brute, "region %s:%d-%d" % (bam.refs[tid][0], beg, end)
        n_hits += len(brute)
    assert n_hits > 0 or not any(rid >= 0 for rid, _, _, _ in iv)


bam_path_of = {}      # id(BamFile) -> its path (for the .bai beside it)


def load(path):
    b = BamFile(path)
    bam_path_of[id(b)] = path
    return b


# ---- 2. the sorted file against the unsorted file of the same library -----------------------------------------------------------
def feed(g, lib, out_dir, batch, attached, se=False, spill_attached=False, halves=False, **dev):
    """One pass over the case's reads in batches of `batch`.  Every batch goes to an unsorted writer (the definition's input) and to sorted writers:
       S   all of it by fq_bam_add_last -- from the attached context (the call sorts its records) or from the host formatter
       P   the same with sort_mem = 1: every run spilled
       H   (halves) even batches by fq_bam_add_last, odd batches as bytes by fq_bam_write_records
    Returns the paths, the stats of every sorted writer and what the feeding implies for them."""
    os.makedirs(out_dir, exist_ok=True)
    names, seq, qual, lens = ob.read_fastq_pair(g["fq1"], g["fq2"])
    if se:
        names, seq, qual, lens = list(names), seq[:1], qual[:1], lens[:1]
    ix = api.Index(g["prefix"], lib=lib, **dev)
    al = api.Aligner(ix, api.default_opts(lib, trim_qual=g["trim_qual"], single_end=1 if se else 0), max_pairs=max(16, batch))
    fai = os.path.join(g["dir"], "genome.fai")
    path = {k: os.path.join(out_dir, k + ".bam") for k in "USPH"}
    U = api.BamWriter(ix, fai, path["U"])
    F = api.BamWriter(ix, fai, None)                     # a formatter without a file: the records as bytes
    S = P = H = None
    if halves:
        H = api.BamWriter(ix, fai, path["H"], sorted=True)
    else:
        S = api.BamWriter(ix, fai, path["S"], sorted=True)
        P = api.BamWriter(ix, fai, path["P"], sorted=True, sort_mem=1)
    fai_refs = [int(l.split("\t")[1]) for l in open(fai) if l.strip()]
    owner = None
    if attached:
        owner = H if halves else (P if spill_attached else S)
        owner.attach(al)
    n = seq.shape[1]
    runs, nonempty, by_add = 0, 0, 0
    for k, lo in enumerate(range(0, n, batch)):
        hi = min(n, lo + batch)
        if halves and attached:                        # the odd batches leave through a formatter of their own
            (H if k % 2 == 0 else F).attach(al)
        al.align(seq[:, lo:hi], qual[:, lo:hi], lens[:, lo:hi], names[lo:hi])
        if halves:
            raw = (H if attached and k % 2 == 0 else F).format_last(al)
            if k % 2 == 0:
                H.add(al); by_add += 1
            else:
                H.write_records(raw)
            U.write_records(raw)
        elif attached:
            owner.add(al)
            raw = owner.format_last(al)                # (input order, as ever: what the workers of --devices hand on)
            U.write_records(raw)
            (S if spill_attached else P).write_records(raw)
        else:
            raw = F.format_last(al)
            U.add(al); S.add(al); P.add(al)
        runs += 1
        nonempty += 1 if raw else 0
        # the run's entries: one per record, stated here from the record bytes; a run that the call sorted arrives in key order, a run of bytes in input order
        w = H if halves else (owner or S)
        ent = [(int(e["key"]), int(e["len"]), int(e["end"])) for e in w.run_entries(-1)]
        recs = split_records(raw)
        n_ref, pos_bits = len(fai_refs), (max(fai_refs) + 1).bit_length()
        want = [(sort_key(r, n_ref, pos_bits), len(r), fields(r)[3]) for r in recs]
        if attached and not (halves and k % 2):
            assert all(a[0] <= b[0] for a, b in zip(ent, ent[1:])), "a run sorted inside its call arrives in key order"
            want.sort(key=lambda t: t[0])
        assert ent == want
    stats = {}
    for k, w in (("S", S), ("P", P), ("H", H)):
        if w is not None:
            live = w.sort_stats()
            w.close()
            stats[k] = w.sort_stats()
            assert all(stats[k][f] == live[f] for f in ("runs", "device_sorted_runs", "spilled_runs", "records", "key_bits"))
            assert stats[k]["close_sec"] > 0
    assert not [f for f in os.listdir(out_dir) if ".tmp." in f], "no spill file may be left behind"
    U.close(); F.close()
    al.close(); ix.close()
    return path, stats, dict(runs=runs, nonempty=nonempty, by_add=by_add, owner="H" if halves else ("P" if spill_attached else "S"))


def check_case(g, lib, tmp, attached, se=False, index_regions=50, quarter=True, **dev):
    tmp = str(tmp)
    B = g["batch"]
    # the golden batch size: S by add_last; P with every run spilled
    path, st, fed = feed(g, lib, os.path.join(tmp, "a"), B, attached, se=se, **dev)
    U = load(path["U"])
    assert len(U.records) > 0
    key_bits = max(1, len(U.refs).bit_length()) + U.pos_bits + 1
    S = check_sorted_against_unsorted(path["S"], U)
    bam_path_of[id(S)] = path["S"]
    check_index(S, index_regions)
    assert load(path["P"]).records == S.records
    for k in "SP":
        assert st[k]["runs"] == fed["runs"] and st[k]["records"] == len(U.records) and st[k]["key_bits"] == key_bits and st[k]["pos_bits"] == U.pos_bits
    assert st["S"]["device_sorted_runs"] == (fed["runs"] if attached else 0) and st["S"]["spilled_runs"] == 0
    assert st["P"]["device_sorted_runs"] == 0 and st["P"]["spilled_runs"] == fed["nonempty"] > 0
    if attached:      # ... and the spilled runs once as the device-sorted runs of the attached context
        path, st, fed = feed(g, lib, os.path.join(tmp, "p"), B, True, se=se, spill_attached=True, **dev)
        assert load(path["P"]).records == S.records
        assert st["P"]["device_sorted_runs"] == st["P"]["runs"] == fed["runs"] and st["P"]["spilled_runs"] == fed["nonempty"] > 0
    # half by fq_bam_add_last, half by fq_bam_write_records
    path, st, fed = feed(g, lib, os.path.join(tmp, "h"), B, attached, se=se, halves=True, **dev)
    assert load(path["U"]).records == U.records
    H = check_sorted_against_unsorted(path["H"], U)
    bam_path_of[id(H)] = path["H"]
    check_index(H, 8, seed=2)
    assert st["H"]["runs"] == fed["runs"] and st["H"]["device_sorted_runs"] == (fed["by_add"] if attached else 0) and st["H"]["spilled_runs"] == 0
    if quarter:       # a quarter of the batch: several runs (the batch size is an input of the alignment: the unsorted file of the SAME feeding is the definition's input)
        Q = max(1, B // 4)
        path, st, fed = feed(g, lib, os.path.join(tmp, "q"), Q, attached, se=se, **dev)
        UQ = load(path["U"])
        SQ = check_sorted_against_unsorted(path["S"], UQ)
        bam_path_of[id(SQ)] = path["S"]
        check_index(SQ, 8, seed=3)
        assert fed["runs"] >= 4 and st["S"]["runs"] == fed["runs"] and st["S"]["device_sorted_runs"] == (fed["runs"] if attached else 0)
        assert load(path["P"]).records == SQ.records and st["P"]["spilled_runs"] == fed["nonempty"]


SIDES = pytest.mark.parametrize("attached", [False, True], ids=["host_formatter", "attached_formatter"])
SE_CONSUMER_TAGS = [t for t in golden_util.se_case_tags() if os.path.exists(os.path.join(golden_util.GOLD, t, "ref_se.bamtxt.gz"))]


@SIDES
@pytest.mark.parametrize("tag", golden_util.case_tags())
def test_sorted_file_is_the_stable_sort_of_the_unsorted_file(tag, attached, golden_cases, emu_lib, tmp_path):
    check_case(golden_cases[tag], emu_lib, tmp_path, attached)


@SIDES
@pytest.mark.parametrize("tag", SE_CONSUMER_TAGS)
def test_single_end_sorted_file_is_the_stable_sort_of_the_unsorted_file(tag, attached, golden_cases, emu_lib, tmp_path):
    check_case(golden_cases[tag], emu_lib, tmp_path, attached, se=True)


def test_an_unsorted_writer_has_no_sort_stats_and_a_sorted_one_needs_a_file(golden_cases, emu_lib, tmp_path):
    g = golden_cases["basic"]
    ix = api.Index(g["prefix"], lib=emu_lib)
    fai = os.path.join(g["dir"], "genome.fai")
    w = api.BamWriter(ix, fai, str(tmp_path / "u.bam"))
    st = api.BamSortStats()
    emu_lib.fq_bam_sort_stats.argtypes = [api.C.c_void_p, api.C.POINTER(api.BamSortStats)]
    assert emu_lib.fq_bam_sort_stats(w.h, api.C.byref(st)) != 0
    w.close()
    with pytest.raises(api.FastquickError):
        api.BamWriter(ix, fai, None, sorted=True)
    # a sorted writer nothing was added to: header, end-of-file block, an index without records
    w = api.BamWriter(ix, fai, str(tmp_path / "empty.bam"), sorted=True)
    with pytest.raises(api.FastquickError):
        w.write_records(b"\x05\x00\x00\x00abcde")      # not whole records
    w.close()
    e = load(str(tmp_path / "empty.bam"))
    assert e.text.startswith(HD_LINE) and not e.records
    bai = Bai(str(tmp_path / "empty.bam.bai"))
    assert bai.n_no_coor == 0 and all(not bins and not lin and pseudo is None for bins, lin, pseudo in bai.refs)
    ix.close()


# ---- 4. the command line ------------------------------------------------------------------------------------------------------------
def write_param(g):
    with open(g["prefix"] + ".param", "w") as fh:
        fh.write("REFERENCE_PATH\t%s\nTARGET_REGION_PATH\tEmpty\nDBSNP_VCF_PATH\tEmpty\nNUM_VAR_LONG\t4\nNUM_VAR_SHORT\t36\n"
                 "SHORT_FLANK_LENGTH\t250\nLONG_FLANK_LENGTH\t1000\n" % os.path.join(g["dir"], "genome"))


def run_cli(exe, g, out, chunk_pairs, *extra, timeout=None, ok=True):
    write_param(g)
    cmd = [exe, "align", "--index_prefix", g["prefix"][:-len(".FASTQuick.fa")], "--fastq_1", g["fq1"], "--fastq_2", g["fq2"], "--out_prefix", out, "--batch_pairs", str(g["batch"]),
           "--chunk_pairs", str(chunk_pairs), "--q", str(g["trim_qual"]), "--read_len", str(g["qc_read_len"])] + list(extra)
    run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    if ok:
        assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    return run


def test_command_line_sorted_bam(golden_cases, emu_cli, tmp_path):
    g = golden_cases["basic"]
    chunk = max(g["batch"], g["n_pairs"] // 3)
    run_cli(emu_cli, g, str(tmp_path / "u"), chunk)
    run = run_cli(emu_cli, g, str(tmp_path / "s"), chunk, "--sorted_bam")
    assert not os.path.exists(str(tmp_path / "s.bam")), "--sorted_bam writes no O.bam"
    U = load(str(tmp_path / "u.bam"))
    S = check_sorted_against_unsorted(str(tmp_path / "s.sorted.bam"), U)
    bam_path_of[id(S)] = str(tmp_path / "s.sorted.bam")
    check_index(S, 50)
    assert b"NOTICE - sorted BAM: %d records in " % len(U.records) in run.stderr and b"close " in run.stderr
    # every run to a file; the host's consumers; both give the same file
    for tag, extra in (("m", ["--sort_mem", "1"]), ("h", ["--host_consumers"])):
        run_cli(emu_cli, g, str(tmp_path / tag), chunk, "--sorted_bam", *extra)
        assert load(str(tmp_path / (tag + ".sorted.bam"))).records == S.records
        assert open(str(tmp_path / (tag + ".sorted.bam.bai")), "rb").read() == open(str(tmp_path / "s.sorted.bam.bai"), "rb").read() or tag == "h"
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]
    bad = run_cli(emu_cli, g, str(tmp_path / "x"), chunk, "--sorted_bam", "--sam_out", ok=False)
    assert bad.returncode != 0 and b"--sam_out" in bad.stderr and not bad.stdout
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("x.")]


def test_command_line_sorted_bam_over_virtual_devices_fq_list_and_single_end(golden_cases, emu_cli, tmp_path):
    g = golden_cases["qc"]
    write_param(g)
    # one pair sharded over two workers: the chunks' records arrive as bytes
    run_cli(emu_cli, g, str(tmp_path / "u"), g["batch"])
    run_cli(emu_cli, g, str(tmp_path / "s2"), g["batch"], "--sorted_bam", "--devices", "0,1")
    U = load(str(tmp_path / "u.bam"))
    S = check_sorted_against_unsorted(str(tmp_path / "s2.sorted.bam"), U)
    bam_path_of[id(S)] = str(tmp_path / "s2.sorted.bam")
    check_index(S, 8)
    # a list of two pairs: one device, and its part files over two
    halves = golden_util.split_halves(g, str(tmp_path))
    lst = str(tmp_path / "two.list")
    with open(lst, "w") as fh:
        fh.write("".join("%s\t%s\n" % h for h in halves))
    base = [emu_cli, "align", "--index_prefix", g["prefix"][:-len(".FASTQuick.fa")], "--batch_pairs", str(g["batch"]), "--chunk_pairs", str(2 * g["batch"]), "--q", str(g["trim_qual"]),
            "--read_len", str(g["qc_read_len"])]
    for out, extra in (("lu", []), ("ls", ["--sorted_bam"]), ("ld", ["--sorted_bam", "--devices", "0,1"])):
        run = subprocess.run(base + ["--fq_list", lst, "--out_prefix", str(tmp_path / out)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    LU = load(str(tmp_path / "lu.bam"))
    LS = check_sorted_against_unsorted(str(tmp_path / "ls.sorted.bam"), LU)
    assert load(str(tmp_path / "ld.sorted.bam")).records == LS.records
    # single-end input
    for out, extra in (("eu", []), ("es", ["--sorted_bam"])):
        run = subprocess.run(base + ["--fastq_1", g["fq1"], "--out_prefix", str(tmp_path / out)] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    check_sorted_against_unsorted(str(tmp_path / "es.sorted.bam"), load(str(tmp_path / "eu.bam")))
    left = [n for n in os.listdir(str(tmp_path)) if ".part" in n or ".worker" in n or ".tmp." in n]
    assert not left, left


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sort_is_the_stable_permutation_on_the_gpu():
    lib = api.load_library()
    check_sort_sizes(lib, SORT_SIZES, device=0)
    rng = np.random.default_rng(7)
    keys = rng.integers(0, 1 << 34, 200003, dtype=np.uint64)      # several workgroups per compute unit's worth of tiles, five passes
    want = np.argsort(keys, kind="stable").astype(np.uint32)
    for _ in range(2):                                             # ... and the same permutation on every run
        perm, ms = api.sort_keys_device(keys, 34, lib=lib, device=0)
        assert (perm == want).all() and ms > 0


@pytest.mark.gpu
@pytest.mark.parametrize("tag,se", [("qc", False), ("wide", False), ("long256", False), ("ragged256", False), (SE_CONSUMER_TAGS[0] if SE_CONSUMER_TAGS else "qc", True)])
def test_sorted_file_on_the_gpu_with_attached_contexts(tag, se, golden_cases, tmp_path):
    lib = api.load_library()
    g = golden_cases[tag]
    check_case(g, lib, tmp_path, True, se=se, index_regions=50, device=0)      # (feed() holds every run's entries to the key order: the call's sort ran, not only the close's)


def make_synth_fastq(tmp):
    """20,000 on-target pairs of 2 x 150 on markers of chromosomes 1, X and Y, a tenth of them random bases (unmapped); index, .param, .fai and the FASTQ pair"""
    from fastquick_amd import synth
    ref = synth.make_reference(n_markers=60, n_long=6, seed=20261018, sex_every=5)
    pre = os.path.join(tmp, "ref.FASTQuick.fa")
    ref.write_fasta(pre)
    api.build_index(pre)
    synth.write_qc_inputs(pre, ref)
    synth.write_param(pre, ref, 6)
    with open(pre + ".genome.fa.fai", "w") as fh:
        fh.write("".join("%s\t%d\t3\t60\t61\n" % (c, len(ref.genome)) for c in ("1", "X", "Y")))
    rb = synth.make_reads(ref, 20000, on_target=0.9, seed=11, sub_rate=0.01, del_frac=0.03, ins_frac=0.03, n_rate=0.001, chimera_frac=0.03, indel_len_max=2)
    fq = []
    for e in range(2):
        fq.append(os.path.join(tmp, "reads_%d.fq" % (e + 1)))
        synth.write_fastq_uniform(rb.seq[e], rb.qual[e], 150, fq[e], bgzf=False)
    return dict(prefix=pre[:-len(".FASTQuick.fa")], fq=fq, out=lambda tag: os.path.join(tmp, tag))


def run_synth(case, tag, extra, env=None):
    cmd = [CLI_GPU, "align", "--index_prefix", case["prefix"], "--fastq_1", case["fq"][0], "--fastq_2", case["fq"][1], "--out_prefix", case["out"](tag), "--read_len", "151"] + extra
    run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=GPU_STEP_SEC, env=dict(os.environ, **(env or {})))
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    return run


@pytest.mark.gpu
def test_command_line_sorted_bam_on_the_gpu(golden_cases, tmp_path):
    """the real FASTQuick_amd align --sorted_bam --chunk_pairs 4096 on seeded synthetic input: one device, every run spilled, two workers on one device; each sorted
    file and index against that command's unsorted O.bam, and the three record streams identical"""
    case = make_synth_fastq(str(tmp_path))
    common = ["--chunk_pairs", "4096", "--batch_pairs", "4096"]      # (a chunk holds whole reference batches: five calls)
    run_synth(case, "u", common)
    U = load(case["out"]("u") + ".bam")
    assert len(U.records) >= 30000 and any(fields(r)[0] < 0 for r in U.records) and len({fields(r)[0] for r in U.records if fields(r)[0] >= 0}) == 3
    streams = []
    for tag, extra in (("s", []), ("m", ["--sort_mem", "1"]), ("d", ["--devices", "0,0"])):
        run = run_synth(case, tag, common + ["--sorted_bam"] + extra)
        path = case["out"](tag) + ".sorted.bam"
        assert not os.path.exists(case["out"](tag) + ".bam")
        S = check_sorted_against_unsorted(path, U)
        bam_path_of[id(S)] = path
        check_index(S, 50)
        streams.append(S.records)
        assert b"NOTICE - sorted BAM:" in run.stderr
        m = re.search(rb"sorted BAM: (\d+) records in (\d+) runs \((\d+) sorted on the device inside their calls, (\d+) spilled", run.stderr)
        n_rec, n_runs, n_dev, n_spill = (int(v) for v in m.groups())
        assert n_rec == len(U.records) and n_runs >= 5
        assert (n_dev, n_spill) == {"s": (n_runs, 0), "m": (n_runs, n_runs), "d": (0, 0)}[tag], "one device: every call sorts its run; --sort_mem 1: every run to a file; workers: runs of bytes"
    assert streams[0] == streams[1] == streams[2]
    # the gather's other form, a thread per sixteen destination bytes (FASTQUICK_BAM_GATHER=pieces is read once per process: a child process of its own): the same file
    run = run_synth(case, "w", common + ["--sorted_bam"], env={"FASTQUICK_BAM_GATHER": "pieces"})
    assert open(case["out"]("w") + ".sorted.bam", "rb").read() == open(case["out"]("s") + ".sorted.bam", "rb").read()
    assert open(case["out"]("w") + ".sorted.bam.bai", "rb").read() == open(case["out"]("s") + ".sorted.bam.bai", "rb").read()
    m = re.search(rb"gather kernels ([0-9.]+) ms", run.stderr)
    assert m and float(m.group(1)) > 0, "the calls' gather kernels are timed and reach the notice"
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f or ".part" in f]
