"""BAM input (`align --bam_in`, fq_frontend_open_bam, fq_bam_transcode_device).

The contract: `--bam_in X` produces what `--fastq_1 T1 --fastq_2 T2` produces, T = transcode(X).  This file holds its own BAM writer and its own
record -> text transcoder, written from the SAM specification 4.2 and the contract; the library is never asked for an expected value.  The CPU
tier runs the host-loop library (tests/emu); the GPU tier runs the same checks on the HIP library, each in a process of its own."""
from __future__ import annotations

import hashlib
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)      # (a GPU check run as a process of its own: `python tests/test_bam_input.py <check>`)

import golden_util  # noqa: E402
from fastquick_amd import api, synth  # noqa: E402

EMU_DIR = os.path.join(ROOT, "tests", "emu")
CHECK_DIR = os.path.join(ROOT, "tests", "bam_input_check")
CLI_GPU = os.path.join(ROOT, "fastquick_amd", "bin", "FASTQuick_amd")
GPU_STEP_SEC = 120      # every GPU step that is a process of its own ends after this long
LETTERS = b"=ACMGRSVTWYHKDBN"
COMPLEMENT = b"=TGKCYSBAWRDMHVN"
CODE_OF = {c: i for i, c in enumerate(LETTERS)}
MAX_BLOCK = 1 << 28
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
QC_FILES = ["AdjustedInsertSizeDist", "DepthDist", "EmpCycleDist", "EmpRepDist", "FASTQ.csv", "GCDist", "InsertSizeTable", "Pileup", "RawInsertSizeDist", "Sequence.csv", "SexChromInfo",
            "Summary", "vcf"]


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "libfq_emu.so"])
    return api.load_library(os.path.join(EMU_DIR, "libfq_emu.so"))


# ---- the BAM writer (SAM specification 4.2) -----------------------------------------------------------------------------------------------
def bam_record(name: bytes, flag: int, codes, quals, ref=-1, pos=-1, mapq=0, cigar=(), next_ref=-1, next_pos=-1, tlen=0, tags=b"", l_seq=None) -> bytes:
    """one alignment record, block_size first; codes: the 4-bit base codes, quals: a byte each; cigar: (op, len) pairs"""
    codes = list(codes)
    n = len(codes) if l_seq is None else l_seq
    packed = bytearray((len(codes) + 1) // 2)
    for i, c in enumerate(codes):
        packed[i >> 1] |= c << (0 if i & 1 else 4)
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1, mapq, 4680, len(cigar), flag, n, next_ref, next_pos, tlen) + name + b"\0"
    body += b"".join(struct.pack("<I", ln << 4 | op) for op, ln in cigar) + bytes(packed) + bytes(quals) + tags
    return struct.pack("<I", len(body)) + body


def bam_header(refs=(("1", 1000),), text="@HD\tVN:1.6\tSO:unsorted\n") -> bytes:
    t = text.encode()
    out = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs))
    for nm, ln in refs:
        out += struct.pack("<i", len(nm) + 1) + nm.encode() + b"\0" + struct.pack("<i", ln)
    return out


def bgzf(data: bytes, member: int = 65280, eof: bool = True) -> bytes:
    out = synth.bgzf_compress(data, threads=2, level=1, member=member)
    assert out.endswith(EOF_BLOCK)
    return out if eof else out[:-len(EOF_BLOCK)]


def fastq_records(path):
    """(name, bases, qualities) of a plain four-line FASTQ file"""
    lines = open(path, "rb").read().split(b"\n")
    return [(lines[i][1:].split()[0], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


def unaligned_bam(reads1, reads2=None, refs=(("1", 1000),)) -> bytes:
    """the reads as an unaligned BAM's payload: flags 77 / 141, or 4 for single-end reads"""
    out = [bam_header(refs)]
    for i, (nm, seq, qual) in enumerate(reads1):
        out.append(bam_record(nm, 77 if reads2 else 4, [CODE_OF[c] for c in seq.upper()], [q - 33 for q in qual]))
        if reads2:
            nm2, seq2, qual2 = reads2[i]
            # (mates share one name in a BAM file: the first mate's, where a golden's FASTQ files name them apart)
            out.append(bam_record(nm, 141, [CODE_OF[c] for c in seq2.upper()], [q - 33 for q in qual2]))
    return b"".join(out)


# ---- the record -> text transcoder (the contract) ---------------------------------------------------------------------------------------
def split_records(payload: bytes, first: int):
    """the chain of whole records from `first`: ([(offset, record bytes)], where the chain ends, how: 0 at the end, 1 inside a record, 2 at a block_size that is none)"""
    recs, p = [], first
    while p < len(payload):
        if p + 4 > len(payload):
            return recs, p, 1
        bs = struct.unpack_from("<I", payload, p)[0]
        if bs < 32 or bs > MAX_BLOCK:
            return recs, p, 2
        if p + 4 + bs > len(payload):
            return recs, p, 1
        recs.append((p, payload[p:p + 4 + bs]))
        p += 4 + bs
    return recs, p, 0


def fields(r: bytes):
    bs, ref, pos, l_name, mapq, bn, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<IiiBBHHHiiii", r, 0)
    return dict(bs=bs, ref=ref, l_name=l_name, n_cig=n_cig, flag=flag, l_seq=l_seq, next_ref=nref)


def record_text(r: bytes) -> bytes:
    f = fields(r)
    nm = r[36:36 + f["l_name"] - 1]
    at = 36 + f["l_name"] + 4 * f["n_cig"]
    l = f["l_seq"]
    packed, qual = r[at:at + (l + 1) // 2], r[at + (l + 1) // 2:at + (l + 1) // 2 + l]
    codes = [(packed[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(l)]
    q = bytes(min(v + 33, 126) for v in qual)
    if f["flag"] & 0x10:
        seq = bytes(COMPLEMENT[c] for c in reversed(codes))
        q = q[::-1]
    else:
        seq = bytes(LETTERS[c] for c in codes)
    return b"@" + nm + b"\n" + seq + b"\n+\n" + q + b"\n"


def record_refusal(r: bytes, paired: bool):
    """what one kept record is refused for on its own: None, or the kind"""
    f = fields(r)
    if bool(f["flag"] & 1) != paired:
        return "mixed"
    if f["l_seq"] == 0:
        return "l_seq0"
    if f["l_seq"] > MAX_BLOCK or f["bs"] < 32 + f["l_name"] + 4 * f["n_cig"] + (f["l_seq"] + 1) // 2 + f["l_seq"]:
        return "fields"
    if f["l_name"] < 2 or any(b < 0x21 or b > 0x7e for b in r[36:36 + f["l_name"] - 1]):
        return "name"
    return None


KIND_RANK = {"mixed": 1, "l_seq0": 2, "fields": 3, "name": 4, "mates": 5, "names": 6}


def transcode(payload: bytes, first: int, paired=None) -> dict:
    """The contract on a payload: texts of the whole pairs (or single records), the first refusal, what is carried."""
    recs, chain_end, end_flag = split_records(payload, first)
    kept = [i for i, (_, r) in enumerate(recs) if not fields(r)["flag"] & 0x900]
    if paired is None:
        paired = bool(kept) and bool(fields(recs[kept[0]][1])["flag"] & 1)
    step = 2 if paired else 1
    n_units = len(kept) // step
    carry_from, used = chain_end, len(recs)
    if paired and len(kept) % 2:
        carry_from, used = recs[kept[-1]][0], kept[-1]
    t, bad = [[], []], []
    for u in range(n_units):
        idx = kept[step * u:step * u + step]
        rs = [recs[i][1] for i in idx]
        ub = [(i, record_refusal(r, paired)) for i, r in zip(idx, rs) if record_refusal(r, paired)]
        if paired:
            fl = [fields(r)["flag"] & 0xc0 for r in rs]
            if not ub and sorted(fl) != [0x40, 0x80]:      # (two records that stand on their own: are they a pair?)
                ub.append((idx[0], "mates"))
            elif not ub and rs[0][36:36 + rs[0][12]] != rs[1][36:36 + rs[1][12]]:
                ub.append((idx[0], "names"))
            if not ub:
                a, b = (0, 1) if fl[0] == 0x40 else (1, 0)
                t[0].append(record_text(rs[a])); t[1].append(record_text(rs[b]))
        elif not ub:
            t[0].append(record_text(rs[0]))
        bad += ub
    first_bad = min(bad, key=lambda x: (x[0], KIND_RANK[x[1]])) if bad else None
    return dict(starts=[o for o, _ in recs], records=len(recs), kept=len(kept), units=n_units, used_records=used, paired=int(paired), chain_end=chain_end, end_flag=end_flag,
                carry_from=carry_from, bad=first_bad, text1=None if bad else b"".join(t[0]), text2=None if bad else b"".join(t[1]))


def check_entry(lib, payload, member_off, first=0, n_ref=1, device=0, what=""):
    want = transcode(payload, first)
    got = api.bam_transcode_device(payload, member_off, n_ref, first, device=device, lib=lib)
    assert got["starts"] == want["starts"], what
    for k in ("records", "kept", "units", "used_records", "chain_end", "end_flag", "carry_from"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    if want["kept"]:
        assert got["paired"] == want["paired"], what
    if want["bad"]:
        assert (got["bad_record"], got["bad_kind"]) == want["bad"], what
    else:
        assert got["bad_record"] == -1 and got["text1"] == want["text1"] and got["text2"] == want["text2"], what
    return got


# ---- 1. the kernel entry against the transcoder --------------------------------------------------------------------------------------------
def rand_read(rng, n, codes=None):
    return (rng.integers(0, 16, n).tolist() if codes is None else [codes[i % len(codes)] for i in range(n)]), rng.integers(0, 60, n).tolist()


def make_pairs(rng, n_pairs, lens=(151,), name_len=12, rev=False, cigar=False, tags=False, n_ref=1):
    out = []
    for p in range(n_pairs):
        nm = (b"%0*d" % (name_len, p))[-name_len:]
        for e in range(2):
            n = lens[(2 * p + e) % len(lens)]
            c, q = rand_read(rng, n)
            flag = (0x41 if e == 0 else 0x81) | (0x10 if rev and (p + e) % 2 else 0)
            tg = b""
            if tags:
                tg = b"RGZgrp" + bytes([p % 200 + 33]) + b"\0" + b"XBBC" + struct.pack("<i", 3) + bytes([1, 2, 3]) + b"XHH1AE3\0" + b"NMC\x05"
            out.append(bam_record(nm, flag, c, q, ref=p % n_ref if cigar else -1, pos=100 + p if cigar else -1, cigar=((4, 3), (0, n - 3)) if cigar and n > 3 else (), next_ref=-1, tags=tg))
    return out


def cuts_with_counts(recs, counts, first=0):
    """member offsets such that the members hold counts[0], counts[1], ... record starts in turn (a last member takes the rest)"""
    at = first
    starts = []
    for r in recs:
        starts.append(at); at += len(r)
    cuts, i = [0], 0
    for c in counts:
        i += c
        if i >= len(starts):
            break
        cuts.append(starts[i] - (7 if len(cuts) % 2 else 0))       # (in front of a record start, or a few bytes inside the record before it)
    return sorted(set(max(0, c) for c in cuts))


def entry_corpus():
    rng = np.random.default_rng(20261018)
    cases = []
    recs = make_pairs(rng, 140, lens=(15, 151, 1, 500), rev=True, cigar=True, tags=True, n_ref=3)
    pay = b"".join(recs)
    cases.append(("counts 0 1 2 63 64 65 per member", pay, cuts_with_counts(recs, [0, 1, 2, 63, 64, 65, 0, 2]), 0, 3))
    for n_mem in (1, 2, 3):
        cases.append(("%d members" % n_mem, pay, [len(pay) * k // n_mem for k in range(n_mem)], 0, 3))
    small = make_pairs(rng, 300, lens=(1, 2, 3), name_len=1)
    ps = b"".join(small)
    for n_mem in (255, 256, 257, 513):      # around the scan's tile of 256
        cases.append(("%d members" % n_mem, ps, sorted(set(len(ps) * k // n_mem for k in range(n_mem))), 0, 1))
    long_names = make_pairs(rng, 6, lens=(16, 17), name_len=254, rev=True)
    cases.append(("names of 254 bytes, odd and even reversed reads", b"".join(long_names), [0, 300, 301, 900], 0, 1))
    # every base code, the qualities at the cap, both strands, odd and even lengths
    allc = []
    for k, l in enumerate((16, 17, 32, 33)):
        for e, fl in enumerate((0x41, 0x81)):
            allc.append(bam_record(b"codes%d" % k, fl | (0x10 if (k + e) % 2 else 0), [(i + e) % 16 for i in range(l)], [(0, 92, 93, 94, 255)[i % 5] for i in range(l)]))
    cases.append(("all codes and qualities", b"".join(allc), [0, 64, 128], 0, 1))
    # skipped records first, last, and between two mates
    a, b = make_pairs(rng, 2, lens=(20,))[:2]
    sec = bam_record(b"sec", 0x141, [1] * 9, [30] * 9)
    sup = bam_record(b"sup", 0x881, [2] * 5, [30] * 5)
    cases.append(("skipped first, between, last", sec + a + sup + sec + b + sup, [0, 50, 100], 0, 1))
    cases.append(("only skipped records", sec + sup + sec, [0, 40], 0, 1))
    # a record spanning three members; members without a record start
    big = bam_record(b"big", 0x41, *rand_read(rng, 700)) + bam_record(b"big", 0x81, *rand_read(rng, 700))
    cases.append(("a record over three members", a + b + big + a + b, [0, 200, 500, 800, 1000, 1300, 1700, 2400], 0, 1))
    # single-end, and a first record behind a header
    se = [bam_record(b"s%d" % i, 4 if i % 3 else 0x14, *rand_read(rng, 30 + i)) for i in range(70)]
    hdr = bam_header((("1", 1000), ("2", 500)))
    cases.append(("single-end behind a header", hdr + b"".join(se), [0, 30, 1000, 2000, 3000], len(hdr), 2))
    cases.append(("no record", hdr, [0], len(hdr), 2))
    cases.append(("empty", b"", [], 0, 1))
    return cases


def check_entry_corpus(lib, device=0):
    for what, pay, cuts, first, n_ref in entry_corpus():
        check_entry(lib, pay, cuts, first, n_ref, device=device, what=what)


def cut_corpus(stride=1):
    """one small record set; the payload ends at every byte in turn, and a member begins at every byte in turn"""
    rng = np.random.default_rng(5)
    recs = make_pairs(rng, 3, lens=(5, 8), name_len=3, tags=True)
    sec = bam_record(b"x", 0x901, [1, 2, 3], [9, 9, 9])
    pay = recs[0] + sec + recs[1] + recs[2] + recs[3] + sec + recs[4] + recs[5]
    out = []
    for cut in range(0, len(pay) + 1, stride):
        out.append(("payload cut at %d" % cut, pay[:cut], [0, cut // 2], 0, 1))
        out.append(("member cut at %d" % cut, pay, [0, cut], 0, 1))
    return out


def check_cut_everywhere(lib, device=0, stride=1):
    for what, pay, cuts, first, n_ref in cut_corpus(stride):
        check_entry(lib, pay, cuts, first, n_ref, device=device, what=what)


def test_kernel_entry_against_the_transcoder(emu_lib):
    check_entry_corpus(emu_lib)


def test_kernel_entry_with_a_cut_at_every_byte(emu_lib):
    check_cut_everywhere(emu_lib)


def test_kernel_entry_with_the_fill_of_sixteen_bytes_a_thread(emu_lib, monkeypatch):
    monkeypatch.setenv("FASTQUICK_BAM_FILL", "pieces")      # (the host-loop launcher reads it at every call; the HIP library once per process)
    check_entry_corpus(emu_lib)
    check_cut_everywhere(emu_lib, stride=5)


# ---- 2. decoys: bytes that pass the validity predicate where no record begins --------------------------------------------------------------
def decoy(n_body: int = 0) -> bytes:
    """36 + n_body bytes that read as a plausible record (fq_bam_plausible1: block_size covers the fields, both reference ids -1, l_read_name 2 with
    its NUL): block_size points a few bytes on, where nothing plausible follows"""
    body = struct.pack("<iiBBHHHiiii", -1, -1, 2, 0, 4680, 0, 0, 1, -1, -1, 0) + b"d\0" + b"\x10" + b"\x05"
    return struct.pack("<I", len(body) + n_body) + body


def decoy_chain(k: int) -> bytes:
    """k decoys whose block_size fields lead to each other: the predicate's look at the next two records passes as well"""
    return decoy() * k


def decoy_corpus():
    """(what, payload, member offsets, the repairs it must take at least): decoys inside tags and qualities with a member beginning at each; a decoy at every
    member start -- more of them than the relaunches a chunk is given, so the serial walk takes over"""
    rng = np.random.default_rng(77)
    d3 = decoy_chain(3)
    assert len(decoy()) == 40
    recs, cuts, at = [], [0], 0
    for p in range(40):
        nm = b"p%03d" % p
        for e, fl in enumerate((0x41, 0x81)):
            where = (p + e) % 3
            c, q = rand_read(rng, 130)
            tg = b""
            if where == 0:
                tg = b"XDBC" + struct.pack("<i", len(d3)) + d3
                off = 36 + len(nm) + 1 + 65 + 130 + 8
            elif where == 1:
                q = list(d3) + q[len(d3):]
                off = 36 + len(nm) + 1 + 65
            else:
                tg = b"XZZ" + bytes(b if b else 1 for b in d3) + b"\0"      # (a Z tag cannot hold NUL: these do not pass the predicate, the members guess right)
                off = 36 + len(nm) + 1 + 65 + 130 + 3
            r = bam_record(nm, fl, c, q, tags=tg)
            assert where == 2 or r[off:off + len(d3)] == d3
            if (p + e) % 2 == 0:
                cuts.append(at + off)
            recs.append(r); at += len(r)
    out = [("decoys in tags, qualities, names", b"".join(recs), cuts, 1)]
    recs, cuts, at = [], [0], 0
    for p in range(150):
        for e, fl in enumerate((0x41, 0x81)):
            c, q = rand_read(rng, 60)
            r = bam_record(b"q%03d" % p, fl, c, list(d3) + q[len(d3):])
            cuts.append(at + 36 + 5 + 30)
            recs.append(r); at += len(r)
    out.append(("a decoy at every member start", b"".join(recs), cuts, 65))
    return out


def check_decoys(lib, device=0):
    for what, pay, cuts, least in decoy_corpus():
        got = check_entry(lib, pay, cuts, device=device, what=what)
        assert got["chain_repairs"] >= least, (what, got["chain_repairs"], "the repair path (and, past 64 relaunches, the serial walk) must have run")


def test_decoys_at_member_starts_are_repaired(emu_lib):
    check_decoys(emu_lib)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------
def refusal_cases():
    """(what, records, (ordinal, kind) of the first refusal, a word of its message)"""
    rng = np.random.default_rng(3)
    P = make_pairs(rng, 4, lens=(20,))
    a0, b0, a1, b1, a2, b2 = P[:6]
    other = bam_record(b"zzzzzzzzzzzz", 0x81, *rand_read(rng, 20))
    first_again = bam_record(b"%012d" % 1, 0x41, *rand_read(rng, 20))
    single = bam_record(b"%012d" % 1, 0x4, *rand_read(rng, 20))
    nobase = bam_record(b"%012d" % 1, 0x81, [], [])
    space = bam_record(b"a name", 0x41, *rand_read(rng, 20))
    space2 = bam_record(b"a name", 0x81, *rand_read(rng, 20))
    sec = bam_record(b"sec", 0x101, [1] * 9, [30] * 9)
    return [("mates not adjacent (sorted by coordinate: both second mates)", [a0, b0, b1, b2, a1, a2], (2, "mates"), "collate the file by name"),
            ("names differ", [a0, b0, a1, other], (2, "names"), "names differ"),
            ("0x40 twice", [a0, b0, sec, a1, first_again], (3, "mates"), "collate the file by name"),
            ("mixed paired and single-end", [a0, b0, a1, single], (3, "mixed"), "mixed"),
            ("l_seq == 0", [a0, b0, a1, nobase], (3, "l_seq0"), "l_seq == 0"),
            ("a name byte 0x20", [a0, b0, space, space2], (2, "name"), "0x21..0x7e")]


def check_refusals_entry(lib, device=0):
    for what, recs, bad, _ in refusal_cases():
        pay = b"".join(recs)
        got = check_entry(lib, pay, [0, len(pay) // 2], device=device, what=what)
        assert (got["bad_record"], got["bad_kind"]) == bad and got["text1"] is None, what


def drain(fe, se):
    """every batch of a front end: per side the heads [3][n], lengths, names"""
    sides = [[[], [], []] for _ in range(1 if se else 2)]
    total = 0
    while True:
        n, b = fe.next()
        assert n != api.FQ_EFALLBACK
        if n == 0:
            break
        head, lens, names = fe.fetch(b, n, se)
        for e in range(len(sides)):
            sides[e][0].append(head[:, e * n:(e + 1) * n].copy()); sides[e][1].append(lens[e * n:(e + 1) * n].copy()); sides[e][2].append(names[e * n:(e + 1) * n].copy())
        total += n
        fe.release(b)
    out = []
    for sd in sides:
        out.append((np.concatenate(sd[0], axis=1), np.concatenate(sd[1]), np.concatenate(sd[2], axis=0)) if sd[0] else None)
    return total, out


def test_refusals_name_the_record(emu_lib, tmp_path, capfd):
    check_refusals_entry(emu_lib)
    hdr = bam_header()
    for k, (what, recs, bad, word) in enumerate(refusal_cases()):
        path = str(tmp_path / ("bad%d.bam" % k))
        open(path, "wb").write(bgzf(hdr + b"".join(recs), member=120))
        fe = api.BamFrontEnd(path, batch_pairs=2, chunk_pairs=4, lib=emu_lib)
        with pytest.raises(api.FastquickError) as ei:
            drain(fe, False)
        fe.close()
        assert "BAM record %d:" % bad[0] in str(ei.value) and word in str(ei.value), (what, str(ei.value))
    good = hdr + b"".join(make_pairs(np.random.default_rng(4), 8, lens=(30,)))
    files = {"magic": (bgzf(b"BAM\2" + good[4:]), "no BAM magic"), "gzip": (__import__("gzip").compress(good), "not a BGZF file"), "header": (bgzf(hdr[:len(hdr) - 5]), "ends inside the header")}
    for tag, (blob, word) in files.items():
        path = str(tmp_path / (tag + ".bam"))
        open(path, "wb").write(blob)
        with pytest.raises(api.FastquickError) as ei:
            api.bam_probe(path, lib=emu_lib)
        assert word in str(ei.value), (tag, str(ei.value))
        with pytest.raises(api.FastquickError):
            api.BamFrontEnd(path, batch_pairs=2, chunk_pairs=4, lib=emu_lib)
    # a stream cut inside a record (at a member boundary: whole members, the last record is not whole)
    path = str(tmp_path / "cutrec.bam")
    open(path, "wb").write(bgzf(good[:len(good) - 11], member=100))
    fe = api.BamFrontEnd(path, batch_pairs=2, chunk_pairs=4, lib=emu_lib)
    with pytest.raises(api.FastquickError) as ei:
        drain(fe, False)
    fe.close()
    assert "ends inside a record (BAM record 15)" in str(ei.value)
    # no end-of-file block: a warning, and every pair is there
    path = str(tmp_path / "noeof.bam")
    open(path, "wb").write(bgzf(good, member=100, eof=False))
    assert api.bam_probe(path, lib=emu_lib)["has_eof_block"] == 0
    capfd.readouterr()
    fe = api.BamFrontEnd(path, batch_pairs=2, chunk_pairs=4, lib=emu_lib)
    n, _ = drain(fe, False)
    fe.close()
    assert n == 8 and "WARNING" in capfd.readouterr().err
    pr = api.bam_probe(str(tmp_path / "bad0.bam"), lib=emu_lib)
    assert pr["n_ref"] == 1 and pr["paired"] == 1 and pr["first_l_seq"] == 20 and pr["sort_order"] == "unsorted" and pr["has_eof_block"] == 1 and pr["header_bytes"] == len(hdr)


# ---- 4. the front end: the batches of a BAM against those of its FASTQ texts ----------------------------------------------------------------
def write_texts(payload, first, tmp, tag):
    """T1 / T2 of a BAM payload as BGZF FASTQ files; (paths, the transcoder's result)"""
    t = transcode(payload, first)
    assert t["bad"] is None and t["end_flag"] == 0 and t["carry_from"] == len(payload)
    paths = []
    for e in range(2 if t["paired"] else 1):
        paths.append(os.path.join(tmp, "%s_T%d.fq.gz" % (tag, e + 1)))
        open(paths[-1], "wb").write(bgzf(t["text%d" % (e + 1)]))
    return paths, t


def check_front_end(lib, bam_payload, first, tmp, tag, batch, chunk, max_len, device=0, members=(65280, 300), modes=(0, 1, 2), headrooms=(None, "0")):
    paths, t = write_texts(bam_payload, first, tmp, tag)
    se = not t["paired"]
    old = os.environ.get("FASTQUICK_FE_HEADROOM")
    try:
        for mode in modes:
            for hr in headrooms:
                if hr is None:
                    os.environ.pop("FASTQUICK_FE_HEADROOM", None)
                else:
                    os.environ["FASTQUICK_FE_HEADROOM"] = hr
                fq = api.DeviceFrontEnd(paths[0], None if se else paths[1], batch_pairs=batch, chunk_pairs=chunk, slot_mode=mode, max_read_len=max_len, device=device, lib=lib)
                n_want, want = drain(fq, se)
                fq.close()
                assert n_want == t["units"]
                for member in members:
                    path = os.path.join(tmp, "%s_%d.bam" % (tag, member))
                    if not os.path.exists(path):
                        open(path, "wb").write(bgzf(bam_payload, member=member))
                    fe = api.BamFrontEnd(path, batch_pairs=batch, chunk_pairs=chunk, slot_mode=mode, max_read_len=max_len, device=device, lib=lib)
                    n_got, got = drain(fe, se)
                    st = fe.stats()
                    fe.close()
                    assert n_got == n_want and st["bam_records"] == t["records"] and st["bam_skipped"] == t["records"] - t["kept"], (tag, mode, hr, member)
                    for e in range(len(want)):
                        for k in range(3):
                            assert got[e][k].shape == want[e][k].shape and (got[e][k] == want[e][k]).all(), (tag, mode, hr, member, e, ("heads", "lengths", "names")[k])
    finally:
        if old is None:
            os.environ.pop("FASTQUICK_FE_HEADROOM", None)
        else:
            os.environ["FASTQUICK_FE_HEADROOM"] = old


def golden_bam(g, se=False):
    r1 = fastq_records(g["fq1"])
    pay = unaligned_bam(r1, None if se else fastq_records(g["fq2"]))
    return pay, len(bam_header()), max(160, (max(len(s) for _, s, _ in r1) + 15) // 16 * 16)


def check_front_end_golden(lib, g, tmp, se, device=0, **kw):
    pay, first, max_len = golden_bam(g, se)
    if not se:
        max_len = max(max_len, (max(len(s) for _, s, _ in fastq_records(g["fq2"])) + 15) // 16 * 16)
    batch = g["batch"]
    check_front_end(lib, pay, first, tmp, ("se_" if se else "pe_") + os.path.basename(g["dir"]), batch, max(batch, g["n_pairs"] // 3 // batch * batch), max_len, device=device, **kw)


@pytest.mark.parametrize("tag", golden_util.case_tags())
def test_front_end_batches_of_a_paired_bam_equal_those_of_its_texts(tag, golden_cases, emu_lib, tmp_path):
    check_front_end_golden(emu_lib, golden_cases[tag], str(tmp_path), False)


@pytest.mark.parametrize("tag", golden_util.se_case_tags())
def test_front_end_batches_of_a_single_end_bam_equal_those_of_its_text(tag, golden_cases, emu_lib, tmp_path):
    check_front_end_golden(emu_lib, golden_cases[tag], str(tmp_path), True)


def synthetic_stream(n_pairs, seed=9, skipped_every=97):
    """an unaligned BAM payload of n_pairs pairs of 2 x 100, reverse-strand and skipped records among them: megabytes, so that its chunks are chunks of payload"""
    rng = np.random.default_rng(seed)
    codes = np.array([1, 2, 4, 8, 15], dtype=np.uint8)[rng.integers(0, 5, (2 * n_pairs, 100))]
    quals = rng.integers(2, 41, (2 * n_pairs, 100), dtype=np.uint8)
    packed = (codes[:, 0::2] << 4 | codes[:, 1::2]).astype(np.uint8)
    out = [bam_header()]
    sec = bam_record(b"skipped", 0x901, [1] * 30, [20] * 30)
    for p in range(n_pairs):
        nm = b"syn%09d" % p
        for e in range(2):
            i = 2 * p + e
            fl = (0x4d if e == 0 else 0x8d) | (0x10 if i % 5 == 0 else 0)
            body = struct.pack("<iiBBHHHiiii", -1, -1, len(nm) + 1, 0, 4680, 0, fl, 100, -1, -1, 0) + nm + b"\0" + packed[i].tobytes() + quals[i].tobytes()
            out.append(struct.pack("<I", len(body)) + body)
            if i % skipped_every == 0:
                out.append(sec)
    return b"".join(out), len(out[0])


def test_front_end_stream_of_several_payload_chunks(emu_lib, tmp_path):
    pay, first = synthetic_stream(12000)
    check_front_end(emu_lib, pay, first, str(tmp_path), "syn", 500, 2000, 160, members=(65280,), modes=(0,), headrooms=(None,))
    fe = api.BamFrontEnd(str(tmp_path / "syn_65280.bam"), batch_pairs=500, chunk_pairs=2000, lib=emu_lib)
    n, _ = drain(fe, False)
    st = fe.stats()
    assert st["chunks"] >= 4 and st["members"] > 60 and n == 12000
    with pytest.raises(api.FastquickError):
        fe.handover()
    fe.close()


# ---- 5. the command line: the defining equality ---------------------------------------------------------------------------------------------
def write_param(g):
    with open(g["prefix"] + ".param", "w") as fh:
        fh.write("REFERENCE_PATH\t%s\nTARGET_REGION_PATH\tEmpty\nDBSNP_VCF_PATH\tEmpty\nNUM_VAR_LONG\t4\nNUM_VAR_SHORT\t36\n"
                 "SHORT_FLANK_LENGTH\t250\nLONG_FLANK_LENGTH\t1000\n" % os.path.join(g["dir"], "genome"))


def run_cli(exe, g, out, inputs, *extra, ok=True, timeout=None, chunk=None):
    write_param(g)
    cmd = [exe, "align", "--index_prefix", g["prefix"][:-len(".FASTQuick.fa")], "--out_prefix", out, "--batch_pairs", str(g["batch"]),
           "--chunk_pairs", str(chunk or max(g["batch"], g["n_pairs"] // 3)), "--q", str(g["trim_qual"]), "--read_len", str(g["qc_read_len"])] + list(inputs) + list(extra)
    run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    if ok:
        assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    return run


def bgzf_payload(path):
    blob, at, parts = open(path, "rb").read(), 0, []
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04"
        bsize = struct.unpack_from("<H", blob, at + 16)[0] + 1
        parts.append(zlib.decompress(blob[at + 18:at + bsize - 8], -15))
        at += bsize
    return b"".join(parts)


def bam_first_record(payload):
    l_text = struct.unpack_from("<i", payload, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", payload, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", payload, at)[0]
    return at, n_ref


def check_cli_equality(exe, g, X_payload, tmp, tag, member=65280, timeout=None, sorted_too=True, qc_needed=True):
    """--bam_in X against --fastq_1 T1 [--fastq_2 T2], T = transcode(X): SAM text, QC files, BAM payload, sorted BAM and index"""
    first, _ = bam_first_record(X_payload)
    paths, t = write_texts(X_payload, first, tmp, tag)
    X = os.path.join(tmp, tag + "_X.bam")
    open(X, "wb").write(bgzf(X_payload, member=member))
    fq_in = ["--fastq_1", paths[0]] + (["--fastq_2", paths[1]] if t["paired"] else [])
    bam_in = ["--bam_in", X]
    sam = [run_cli(exe, g, os.path.join(tmp, tag + k), inp, "--sam_out", timeout=timeout) for k, inp in (("_sf", fq_in), ("_sb", bam_in))]
    assert sam[0].stdout == sam[1].stdout and any(ln and not ln.startswith(b"@") for ln in sam[0].stdout.split(b"\n")), tag      # (equal, and records among the lines)
    assert b"NOTICE - BAM input on the device: %d records (%d skipped" % (t["records"], t["records"] - t["kept"]) in sam[1].stderr, sam[1].stderr.decode()[-2000:]
    n_qc = 0
    for name in QC_FILES:
        fa, fb = (os.path.join(tmp, tag + k + "." + name) for k in ("_sf", "_sb"))
        if not os.path.exists(fa):
            continue
        a, b = open(fa, "rb").read(), open(fb, "rb").read()
        if name == "FASTQ.csv":
            for pth in paths:
                a = a.replace(os.path.basename(pth).encode(), os.path.basename(X).encode())
        assert a == b, (tag, name)
        n_qc += 1
    assert n_qc == (13 if qc_needed else 0), "the QC files are written where the index carries its sites"
    runs = [("_uf", fq_in, []), ("_ub", bam_in, [])] + ([("_of", fq_in, ["--sorted_bam"]), ("_ob", bam_in, ["--sorted_bam"])] if sorted_too else [])
    for k, inp, extra in runs:
        run_cli(exe, g, os.path.join(tmp, tag + k), inp, *extra, timeout=timeout)
    assert bgzf_payload(os.path.join(tmp, tag + "_uf.bam")) == bgzf_payload(os.path.join(tmp, tag + "_ub.bam")), tag
    if sorted_too:
        assert bgzf_payload(os.path.join(tmp, tag + "_of.sorted.bam")) == bgzf_payload(os.path.join(tmp, tag + "_ob.sorted.bam")), tag
        assert open(os.path.join(tmp, tag + "_of.sorted.bam.bai"), "rb").read() == open(os.path.join(tmp, tag + "_ob.sorted.bam.bai"), "rb").read(), tag
    return os.path.join(tmp, tag + "_ub.bam")


def splice_skipped(payload):
    """secondary and supplementary copies of some records spliced in: in front of the first, between mates, behind the last"""
    first, _ = bam_first_record(payload)
    recs, end, flag = split_records(payload, first)
    assert flag == 0 and end == len(payload)
    out = [payload[:first]]
    for i, (_, r) in enumerate(recs):
        copy = bytearray(r)
        struct.pack_into("<H", copy, 18, (struct.unpack_from("<H", r, 18)[0] | (0x100 if i % 2 else 0x800)))
        if i % 7 == 0:
            out.append(bytes(copy))
        out.append(r)
    out.append(bytes(copy))
    return b"".join(out)


def check_cli_golden(exe, g, tmp, timeout=None, full=True):
    pay, _, _ = golden_bam(g)
    out_bam = check_cli_equality(exe, g, pay, tmp, "unaln", timeout=timeout)
    if not full:
        return
    check_cli_equality(exe, g, pay, tmp, "small", member=300, timeout=timeout, sorted_too=False)
    fed = bgzf_payload(out_bam)      # the O.bam this command line wrote: reverse-strand records, CIGARs, tags
    assert any(struct.unpack_from("<H", r, 18)[0] & 0x10 for _, r in split_records(fed, bam_first_record(fed)[0])[0])
    check_cli_equality(exe, g, fed, tmp, "fed", timeout=timeout, sorted_too=False)
    check_cli_equality(exe, g, splice_skipped(fed), tmp, "spliced", member=4000, timeout=timeout, sorted_too=False)
    se_pay, _, _ = golden_bam(g, se=True)
    check_cli_equality(exe, g, se_pay, tmp, "single", timeout=timeout, sorted_too=False)


def test_command_line_bam_in_equals_the_fastq_run_on_its_texts(golden_cases, emu_cli, tmp_path):
    check_cli_golden(emu_cli, golden_cases["qc"], str(tmp_path))


@pytest.mark.parametrize("tag", golden_util.case_tags())
def test_command_line_equality_on_every_paired_golden_as_an_unaligned_bam(tag, golden_cases, emu_cli, tmp_path):
    g = golden_cases[tag]
    check_cli_equality(emu_cli, g, golden_bam(g)[0], str(tmp_path), "unaln", sorted_too=False, qc_needed=os.path.exists(g["prefix"] + ".SelectedSite.vcf"))


@pytest.mark.parametrize("tag", golden_util.se_case_tags())
def test_command_line_equality_on_every_single_end_golden_as_an_unaligned_bam(tag, golden_cases, emu_cli, tmp_path):
    g = golden_cases[tag]
    check_cli_equality(emu_cli, g, golden_bam(g, se=True)[0], str(tmp_path), "single", sorted_too=False, qc_needed=os.path.exists(g["prefix"] + ".SelectedSite.vcf"))


def test_a_read_longer_than_the_rows_is_an_error_not_a_hand_over(emu_lib, tmp_path):
    rng = np.random.default_rng(8)
    recs = make_pairs(rng, 12, lens=(100,))
    recs[14] = bam_record(b"%012d" % 7, 0x41, *rand_read(rng, 200))      # pair 7's first mate: longer than the rows of 160
    path = str(tmp_path / "long.bam")
    open(path, "wb").write(bgzf(bam_header() + b"".join(recs)))
    fe = api.BamFrontEnd(path, batch_pairs=4, chunk_pairs=4, max_read_len=160, lib=emu_lib)
    got = 0
    while True:
        n, b = fe.next() if got < 4 else (fe.L.fq_frontend_next(fe.h, api.C.byref(api.C.c_void_p())), None)
        if n <= 0:
            break
        got += n
        fe.release(b)
    assert got == 4 and n == -5 and n != api.FQ_EFALLBACK, (got, n)      # FQ_ELIMIT behind the whole reference batches in front of the read
    msg = fe.L.fq_frontend_last_error(fe.h).decode()
    assert "longer than the rows (160 bases" in msg and "long.bam" in msg, msg
    with pytest.raises(api.FastquickError):
        fe.handover()
    fe.close()


def test_command_line_refuses_what_bam_input_cannot_be_combined_with(golden_cases, emu_cli, tmp_path):
    g = golden_cases["basic"]
    pay, _, _ = golden_bam(g)
    X = str(tmp_path / "x.bam")
    open(X, "wb").write(bgzf(pay))
    lst = str(tmp_path / "l.list")
    open(lst, "w").write("%s\t%s\n" % (g["fq1"], g["fq2"]))
    for extra, word in ((["--fastq_1", g["fq1"]], b"--fastq_1"), (["--fastq_2", g["fq2"]], b"--fastq_1"), (["--fq_list", lst], b"--fq_list"), (["--host_reader"], b"--host_reader"),
                        (["--frac_samp", "0.5"], b"--frac_samp"), (["--devices", "0,1"], b"--devices")):
        run = run_cli(emu_cli, g, str(tmp_path / "r"), ["--bam_in", X], *extra, ok=False)
        assert run.returncode != 0 and b"--bam_in" in run.stderr and word in run.stderr and not run.stdout, extra
    run = run_cli(emu_cli, g, str(tmp_path / "ok"), ["--bam_in", X], "--devices", "0", "--frac_samp", "1")
    assert run.returncode == 0
    # a coordinate-sorted file: refused, and the message says why
    recs, _, _ = split_records(pay, len(bam_header()))
    srt = bam_header(text="@HD\tVN:1.6\tSO:coordinate\n") + b"".join(r for _, r in recs[0::2]) + b"".join(r for _, r in recs[1::2])
    open(X, "wb").write(bgzf(srt))
    run = run_cli(emu_cli, g, str(tmp_path / "c"), ["--bam_in", X], ok=False)
    assert run.returncode != 0 and b"mates are not adjacent: collate the file by name first" in run.stderr and b"BAM record 0:" in run.stderr


# ---- 6. the host code under AddressSanitizer / UBSan: a program of its own ----------------------------------------------------------------
def write_check_corpus(path):
    """cases 1-3's corpus -- the entry corpus, the cut at every byte, the decoys (with the repairs each must take at least), the refusals -- with the
    transcoder's results, as the check program reads it"""
    cases = [(w, p, c, f, n, 0) for w, p, c, f, n in entry_corpus() + cut_corpus()]
    cases += [(w, p, c, 0, 1, least) for w, p, c, least in decoy_corpus()]
    for what, recs, _, _ in refusal_cases():
        pay = b"".join(recs)
        cases.append((what, pay, [0, len(pay) // 2], 0, 1, 0))
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for what, pay, cuts, first, n_ref, least_repairs in cases:
            t = transcode(pay, first)
            bad = t["bad"] or (-1, None)
            t1, t2 = t["text1"] or b"", t["text2"] or b""
            fh.write(struct.pack("<iqqI", n_ref, first, len(pay), len(cuts)) + pay + struct.pack("<%dq" % len(cuts), *cuts))
            fh.write(struct.pack("<qiiqqqqI", bad[0], KIND_RANK.get(bad[1], 0), least_repairs, t["chain_end"], t["carry_from"], len(t1), len(t2), len(t["starts"])) + t1 + t2 + struct.pack("<%dI" % len(t["starts"]), *t["starts"]))
    return len(cases)


def test_host_code_under_sanitizers(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CHECK_DIR, "bam_input_check"])
    corpus = str(tmp_path / "corpus.bin")
    n_cases = write_check_corpus(corpus)
    pay, _ = synthetic_stream(12000)
    bam = str(tmp_path / "stream.bam")
    open(bam, "wb").write(bgzf(pay))
    run = subprocess.run([os.path.join(CHECK_DIR, "bam_input_check"), corpus, bam, "500", "2000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    assert b"ok: %d cases, 12000 pairs" % n_cases in run.stdout, run.stdout


# ---- 7. GPU tier: every check a process of its own under a time limit -------------------------------------------------------------------------
def gpu_step(*args, env=None):
    run = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=GPU_STEP_SEC, env=dict(os.environ, **(env or {})))
    assert run.returncode == 0, (run.stdout.decode(errors="replace")[-1500:], run.stderr.decode(errors="replace")[-3000:])
    return run


@pytest.mark.gpu
def test_kernel_entry_on_the_gpu():
    gpu_step("entry")


@pytest.mark.gpu
def test_decoys_and_refusals_on_the_gpu():
    gpu_step("decoys")


@pytest.mark.gpu
def test_fill_of_sixteen_bytes_a_thread_on_the_gpu():
    gpu_step("entry", env={"FASTQUICK_BAM_FILL": "pieces"})


@pytest.mark.gpu
@pytest.mark.parametrize("tag,se", [("qc", False), ("ragged256", False), ("long250", True)])
def test_front_end_on_the_gpu(tag, se, golden_cases, tmp_path):
    gpu_step("frontend", golden_cases[tag]["dir"], tag, int(se), str(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["qc", "wide"])
def test_command_line_on_the_gpu(tag, golden_cases, tmp_path):
    check_cli_golden(CLI_GPU, golden_cases[tag], str(tmp_path), timeout=GPU_STEP_SEC, full=tag == "qc")


@pytest.mark.gpu
def test_command_line_stream_of_three_chunks_on_the_gpu(tmp_path):
    """100,000 seeded synthetic pairs cut into three chunks: the digest of the SAM text of --bam_in X equals that of the FASTQ run on transcode(X)"""
    tmp = str(tmp_path)
    ref = synth.make_reference(n_markers=60, n_long=6, seed=20261018, sex_every=5)
    pre = os.path.join(tmp, "ref.FASTQuick.fa")
    ref.write_fasta(pre)
    api.build_index(pre)
    synth.write_qc_inputs(pre, ref)
    synth.write_param(pre, ref, 6)
    rb = synth.make_reads(ref, 100000, on_target=0.9, seed=11, sub_rate=0.01, del_frac=0.03, ins_frac=0.03, n_rate=0.001, chimera_frac=0.03, indel_len_max=2)
    code_of = np.zeros(256, dtype=np.uint8)
    for c, i in CODE_OF.items():
        code_of[c] = i
    fq, packed = [], []
    for e in range(2):
        fq.append(os.path.join(tmp, "T%d.fq.gz" % (e + 1)))
        synth.write_fastq_uniform(rb.seq[e], rb.qual[e], 150, fq[e], bgzf=True)
        c = code_of[rb.seq[e][:, :150]]
        packed.append((c[:, 0::2] << 4 | c[:, 1::2]).astype(np.uint8))
    out = [bam_header()]
    for p in range(100000):
        nm = b"r%09d" % p
        for e in range(2):
            body = struct.pack("<iiBBHHHiiii", -1, -1, len(nm) + 1, 0, 4680, 0, 77 if e == 0 else 141, 150, -1, -1, 0) + nm + b"\0" + packed[e][p].tobytes() + (rb.qual[e][p, :150] - 33).astype(np.uint8).tobytes()
            out.append(struct.pack("<I", len(body)) + body)
    X = os.path.join(tmp, "X.bam")
    open(X, "wb").write(bgzf(b"".join(out)))
    digests = []
    for inp in (["--fastq_1", fq[0], "--fastq_2", fq[1]], ["--bam_in", X]):
        cmd = [CLI_GPU, "align", "--index_prefix", pre[:-len(".FASTQuick.fa")], "--out_prefix", os.path.join(tmp, "o%d" % len(digests)), "--read_len", "151", "--sam_out",
               "--chunk_pairs", "36864", "--batch_pairs", "4096"] + inp
        run = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=GPU_STEP_SEC)
        assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
        assert run.stdout.count(b"\n") > 100000
        digests.append(hashlib.sha256(run.stdout).hexdigest())
    assert digests[0] == digests[1]
    assert b"NOTICE - BAM input on the device: 200000 records (0 skipped" in run.stderr


if __name__ == "__main__":
    lib = api.load_library()
    what = sys.argv[1]
    if what == "entry":
        check_entry_corpus(lib)
        check_cut_everywhere(lib, stride=3)
    elif what == "decoys":
        check_decoys(lib)
        check_refusals_entry(lib)
    elif what == "frontend":
        g = golden_util.case_params(sys.argv[3])
        d = sys.argv[2]
        g.update(dir=d, fq1=os.path.join(d, "reads_1.fq"), fq2=os.path.join(d, "reads_2.fq"))
        check_front_end_golden(lib, g, sys.argv[5], bool(int(sys.argv[4])))
    else:
        raise SystemExit("unknown check " + what)
    print("ok")
