"""BAM input with collation (`align --bam_in S.bam --collate`, fq_frontend_open_bam_collate, fq_bam_collate_device).

The contract: `--bam_in S --collate` produces what `--bam_in C` produces, where C holds S's header and the records a serial walk over S emits -- a
dictionary name -> waiting record, pairs in the order of their later mate.  The walk below is written from that definition; expected texts are
test_bam_input's transcoder applied to C; the library is never asked for an expected value.  The CPU tier runs the host-loop library (tests/emu);
the GPU tier runs the same checks on the HIP library, each in a process of its own."""
from __future__ import annotations

import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)      # (a GPU check run as a process of its own: `python tests/test_bam_collate.py <check>`)

import golden_util  # noqa: E402
import test_bam_input as tbi  # noqa: E402
from fastquick_amd import api  # noqa: E402

CHECK_DIR = os.path.join(ROOT, "tests", "bam_collate_check")
KIND_RANK = dict(tbi.KIND_RANK, dup=7)
HASH_BITS = (None, "4", "1", "0")      # FASTQUICK_BAM_HASH_BITS: unset, and many / all names in one run of equal hashes
MEMBER = 300                           # the chunked runs: one member of this many bytes a chunk


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", tbi.EMU_DIR, "libfq_emu.so"])
    return api.load_library(os.path.join(tbi.EMU_DIR, "libfq_emu.so"))


# ---- the yardstick: the definition's walk ---------------------------------------------------------------------------------------------------
def walk(payload: bytes, first: int) -> dict:
    """C's record order, the orphans and the first refusal of the stream payload[first:], by the serial definition"""
    recs, chain_end, end_flag = tbi.split_records(payload, first)
    flags = [tbi.fields(r)["flag"] for _, r in recs]
    kept = [i for i, f in enumerate(flags) if not f & 0x900]
    paired = bool(kept) and bool(flags[kept[0]] & 1)
    out = dict(records=len(recs), kept=len(kept), paired=int(paired), chain_end=chain_end, end_flag=end_flag)
    if not paired:      # --collate changes nothing
        t = tbi.transcode(payload, first)
        out.update(order=kept, orphans=[], bad=t["bad"], pairs=t["units"], C=payload)
        return out
    waiting, order, bad = {}, [], []
    for i in kept:
        r = recs[i][1]
        kind = tbi.record_refusal(r, True)
        if kind is None and flags[i] & 0xc0 not in (0x40, 0x80):
            kind = "mates"
        if kind:
            bad.append((i, kind))
            continue
        name = r[36:36 + r[12]]      # (l_read_name bytes: the length is part of the key)
        w = waiting.get(name)
        if w is None:
            waiting[name] = i
        elif (flags[w] ^ flags[i]) & 0xc0 == 0:
            bad.append((i, "dup"))
        else:
            order += [w, i] if flags[w] & 0x40 else [i, w]
            del waiting[name]
    out.update(order=order, orphans=sorted(waiting.values()), bad=min(bad, key=lambda x: (x[0], KIND_RANK[x[1]])) if bad else None, pairs=len(order) // 2,
               C=payload[:first] + b"".join(recs[i][1] for i in order))
    return out


def check_collate(lib, payload, first=0, n_ref=1, per_chunk=0, device=0, what="", member=MEMBER):
    want = walk(payload, first)
    cuts = list(range(0, len(payload), member))
    got = api.bam_collate_device(payload, cuts, n_ref, first, members_per_chunk=per_chunk, device=device, lib=lib)
    tag = (what, per_chunk, os.environ.get("FASTQUICK_BAM_HASH_BITS"))
    if want["bad"]:
        assert (got["bad_record"], got["bad_kind"]) == want["bad"], (tag, got["bad_record"], got["bad_kind"], want["bad"])
        return got
    t = tbi.transcode(want["C"], first)
    assert t["bad"] is None
    assert got["bad_record"] == -1, (tag, got["bad_record"], got["bad_kind"])
    assert got["records"] == want["records"] and got["kept"] == want["kept"], tag
    assert got["pairs"] == want["pairs"] and (not want["paired"] or got["orphans"] == len(want["orphans"])), (tag, got["pairs"], want["pairs"], got["orphans"], len(want["orphans"]))
    assert got["text1"] == t["text1"] and got["text2"] == (t["text2"] or b""), tag
    assert got["held_peak_records"] >= got["orphans"], tag
    if per_chunk:
        assert got["chunks"] >= min(5, (len(payload) - first) // member), tag
    return got


# ---- 1. the kernel entry ------------------------------------------------------------------------------------------------------------------------
def rec(rng, name: bytes, side: int, l=20, extra=0, **kw):
    return tbi.bam_record(name, (0x41 if side == 1 else 0x81) | extra, *tbi.rand_read(rng, l), **kw)


def apart(rng, d, tag=b"f"):
    """the mates of pair A d kept records apart: d - 1 first mates of other pairs between them, whose second mates follow"""
    fill = [tag + b"%04d" % k for k in range(d - 1)]
    return [rec(rng, b"A", 1)] + [rec(rng, nm, 1) for nm in fill] + [rec(rng, b"A", 2)] + [rec(rng, nm, 2) for nm in fill]


def good_cases():
    """(what, records, header or b"")"""
    rng = np.random.default_rng(20261019)
    R = lambda nm, side, **kw: rec(rng, nm, side, **kw)      # noqa: E731
    cases = [("one pair adjacent", [R(b"A", 1), R(b"A", 2)]), ("one pair, the 0x80 record first", [R(b"A", 2), R(b"A", 1)])]
    for d in (1, 2, 63, 64, 65, 255, 256, 257):
        cases.append(("mates %d kept records apart" % d, apart(rng, d)))
    cases.append(("nested", [R(b"A", 1), R(b"B", 2), R(b"B", 1), R(b"A", 2)]))
    cases.append(("crossing", [R(b"A", 1), R(b"B", 1), R(b"A", 2), R(b"B", 2)]))
    # records of ~130 bytes, chunks of 300: every mate below waits over two chunk boundaries at least (three consecutive chunks have a predecessor that holds it)
    far = []
    for k in range(4):
        far += [R(b"far%d" % k, 1 + k % 2, l=60)] + [R(b"pad%d_%d" % (k, j), s, l=60) for j in range(5) for s in (1, 2)]
    far += [R(b"far%d" % k, 2 - k % 2, l=60) for k in range(4)]
    cases.append(("held across chunk boundaries", far))
    # the third record is cut by the first chunk's end (offsets 2 x ~103 bytes .. 300); its mate comes five records later
    cases.append(("a record cut by the payload's end waits for its mate", [R(b"x0", 1, l=40), R(b"x0", 2, l=40), R(b"cut", 2, l=40)] + [R(b"y%d" % j, s, l=40) for j in range(2) for s in (1, 2)] +
                  [R(b"cut", 1, l=40)]))
    cases.append(("skipped records of a waiting name between the mates", [R(b"A", 1), R(b"A", 1, extra=0x800), R(b"B", 2), R(b"A", 2, extra=0x100), R(b"A", 1, extra=0x900), R(b"A", 2), R(b"B", 1),
                                                                          R(b"B", 1, extra=0x800)]))
    cases.append(("names r1 and r10", [R(b"r1", 1), R(b"r10", 1), R(b"r10", 2), R(b"r1", 2)]))
    cases.append(("names that differ in the last byte", [R(b"nameX", 1), R(b"nameY", 1), R(b"nameZ", 2), R(b"nameY", 2), R(b"nameX", 2), R(b"nameZ", 1)]))
    long_a, long_b = b"n" * 253 + b"a", b"n" * 253 + b"b"
    cases.append(("names of 254 bytes", [R(long_a, 1), R(long_b, 2), R(long_a, 2), R(long_b, 1)]))
    cases.append(("a name recurs once its pair is complete", [R(b"A", 1), R(b"A", 2), R(b"A", 1), R(b"A", 2), R(b"A", 2), R(b"B", 1), R(b"A", 1), R(b"B", 2)]))
    full = tbi.make_pairs(rng, 40, lens=(15, 151, 1, 33), rev=True, cigar=True, tags=True, n_ref=3)
    cases.append(("both strands, CIGARs, tags", [full[i] for i in rng.permutation(len(full))]))
    cases.append(("one orphan in the middle", [R(b"A", 1), R(b"orphan", 2), R(b"A", 2), R(b"B", 2), R(b"B", 1)]))
    cases.append(("the last record an orphan", [R(b"A", 1), R(b"A", 2), R(b"orphan", 1)]))
    cases.append(("every record an orphan", [R(b"o%d" % k, 1 + k % 2) for k in range(7)]))
    cases.append(("mates adjacent throughout", tbi.make_pairs(rng, 9, lens=(30,))))
    cases.append(("single-end: the flag changes nothing", [tbi.bam_record(b"s%d" % i, 4 if i % 3 else 0x14, *tbi.rand_read(rng, 30 + i)) for i in range(12)]))
    out = [(w, b"".join(rs), 0, 1) for w, rs in cases]
    hdr = tbi.bam_header((("1", 1000), ("2", 500)))
    out.append(("behind a header", hdr + b"".join(apart(rng, 5)), len(hdr), 2))
    out.append(("no record", hdr, len(hdr), 2))
    return out


def refusal_cases():
    """(what, payload, (ordinal, kind))"""
    rng = np.random.default_rng(31)
    R = lambda nm, side, **kw: rec(rng, nm, side, **kw)      # noqa: E731
    both = tbi.bam_record(b"A", 0xc1, *tbi.rand_read(rng, 20))
    neither = tbi.bam_record(b"A", 0x01, *tbi.rand_read(rng, 20))
    nobase = tbi.bam_record(b"A", 0x81, [], [])
    pad = [R(b"p%d" % j, s, l=50) for j in range(4) for s in (1, 2)]
    cases = [("A/1 A/1", [R(b"A", 1), R(b"A", 1)], (1, "dup")),
             ("A/1 B/1 A/1", [R(b"A", 1), R(b"B", 1), R(b"A", 1)], (2, "dup")),
             ("A/2 ... A/2 over chunk boundaries", [R(b"A", 2)] + pad + [R(b"A", 2), R(b"A", 1)], (9, "dup")),
             ("a record with 0xc0", [R(b"B", 1), both, R(b"B", 2)], (1, "mates")),
             ("a record with neither side bit", [R(b"B", 1), R(b"B", 2), neither], (2, "mates")),
             ("l_seq == 0 on a record whose mate comes first", [R(b"A", 1), R(b"B", 1), nobase, R(b"B", 2)], (2, "l_seq0")),
             ("two refusals in one chunk: the smaller wins", [R(b"A", 1), nobase, R(b"A", 1)], (1, "l_seq0")),
             ("two refusals in one chunk: the duplicate first", [R(b"B", 2), R(b"B", 2), both], (1, "dup")),
             ("a single-end record in a paired stream", [R(b"A", 1), tbi.bam_record(b"A", 0x4, *tbi.rand_read(rng, 20))], (1, "mixed")),
             ("a skipped record is no duplicate", [R(b"A", 1), R(b"A", 1, extra=0x800), R(b"A", 1)], (2, "dup"))]
    return [(w, b"".join(rs), bad) for w, rs, bad in cases]


def seeded_stream(n_pairs=2000, seed=20261019, l_seq=100, far_frac=0.02, sup_frac=0.03, orphan_frac=0.01, mean_dist=30.0, header=True):
    """A coordinate-like permutation of n_pairs pairs: the second mate lies a geometric number of places behind the first, far_frac of them anywhere;
    sup_frac supplementary copies (they carry their primary's name); orphan_frac of the pairs lose a mate; names of 8-40 bytes.  (payload, first)"""
    rng = np.random.default_rng(seed)
    codes = np.array([1, 2, 4, 8, 15], dtype=np.uint8)[rng.integers(0, 5, (2 * n_pairs, l_seq))]
    quals = rng.integers(2, 41, (2 * n_pairs, l_seq), dtype=np.uint8)
    packed = (codes[:, 0::2] << 4 | codes[:, 1::2]).astype(np.uint8)
    where = np.empty(2 * n_pairs)
    where[0::2] = np.arange(n_pairs) * 2.0
    where[1::2] = where[0::2] + 2.0 * rng.geometric(1.0 / mean_dist, n_pairs) - 0.5
    far = rng.random(n_pairs) < far_frac
    where[1::2][far] = rng.random(int(far.sum())) * 2.0 * n_pairs
    lost = rng.random(n_pairs) < orphan_frac
    name_len = rng.integers(8, 41, n_pairs)
    out = [tbi.bam_header()] if header else [b""]
    for i in np.argsort(where, kind="stable"):
        p, e = int(i) // 2, int(i) % 2
        if lost[p] and e == p % 2:
            continue
        nm = (b"q%d_" % p + b"x" * 40)[:int(name_len[p])]
        fl = (0x41 if e == 0 else 0x81) | (0x10 if i % 5 == 0 else 0)
        body = struct.pack("<iiBBHHHiiii", 0, 2 * p, len(nm) + 1, 0, 4680, 0, fl, l_seq, 0, 2 * p, 0) + nm + b"\0" + packed[i].tobytes() + quals[i].tobytes()
        out.append(struct.pack("<I", len(body)) + body)
        if rng.random() < sup_frac:
            body = struct.pack("<iiBBHHHiiii", 0, 7, len(nm) + 1, 0, 4680, 0, fl | 0x800, 10, -1, -1, 0) + nm + b"\0" + bytes(5) + bytes(10)
            out.append(struct.pack("<I", len(body)) + body)
    return b"".join(out), len(out[0])


def check_entry_corpus(lib, device=0, seeded=True):
    for per in (0, 1):
        for what, pay, first, n_ref in good_cases():
            check_collate(lib, pay, first, n_ref, per, device=device, what=what)
        for what, pay, bad in refusal_cases():
            assert walk(pay, 0)["bad"] == bad, what      # (the walk itself against the case's statement)
            check_collate(lib, pay, 0, 1, per, device=device, what=what)
        if seeded:
            pay, first = seeded_stream()
            got = check_collate(lib, pay, first, 1, per, device=device, what="seeded stream")
            assert got["orphans"] >= 10 and got["records"] - got["kept"] >= 60 and got["pairs"] >= 1900
            if per:
                assert got["held_peak_records"] > got["orphans"]


def check_collate_mem(lib, device=0):
    """collate_mem 4096 on the seeded stream: FQ_ELIMIT, the message names the option (nothing written past a buffer: api.bam_collate_device's guard bytes)"""
    pay, first = seeded_stream()
    cuts = list(range(0, len(pay), 4096))
    for per in (0, 1):
        with pytest.raises(api.FastquickError) as ei:
            api.bam_collate_device(pay, cuts, 1, first, members_per_chunk=per, collate_mem=4096, device=device, lib=lib)
        assert ei.value.code == -5 and "--collate_mem" in str(ei.value) and "BAM record" in str(ei.value), str(ei.value)
    # ... and a bound that the waiting records just fit is no error
    got = api.bam_collate_device(pay, cuts, 1, first, members_per_chunk=1, device=device, lib=lib)
    again = api.bam_collate_device(pay, cuts, 1, first, members_per_chunk=1, collate_mem=got["held_peak_bytes"], device=device, lib=lib)
    assert again["pairs"] == got["pairs"] and again["text1"] == got["text1"]
    with pytest.raises(api.FastquickError):
        api.bam_collate_device(pay, cuts, 1, first, members_per_chunk=1, collate_mem=got["held_peak_bytes"] - 1, device=device, lib=lib)


@pytest.mark.parametrize("bits", HASH_BITS)
def test_kernel_entry_against_the_walk(bits, emu_lib, monkeypatch):
    if bits is None:
        monkeypatch.delenv("FASTQUICK_BAM_HASH_BITS", raising=False)
    else:
        monkeypatch.setenv("FASTQUICK_BAM_HASH_BITS", bits)      # (the host-loop library reads it at every call; the HIP library once per process)
    check_entry_corpus(emu_lib)


def test_collate_mem_bounds_the_held_store(emu_lib):
    check_collate_mem(emu_lib)


# ---- 2. the front end: the batches of S with collation against those of C without ---------------------------------------------------------------
def shuffle_like_the_seeded_stream(payload, first, seed=5):
    """the records of an unaligned BAM (mates adjacent) in a coordinate-like order: second mates a geometric distance behind, 2 % anywhere, 1 % lost"""
    recs, end, flag = tbi.split_records(payload, first)
    assert flag == 0 and end == len(payload) and len(recs) % 2 == 0
    rng = np.random.default_rng(seed)
    n = len(recs) // 2
    where = np.empty(2 * n)
    where[0::2] = np.arange(n) * 2.0
    where[1::2] = where[0::2] + 2.0 * rng.geometric(1.0 / 30.0, n) - 0.5
    far = rng.random(n) < 0.02
    where[1::2][far] = rng.random(int(far.sum())) * 2.0 * n
    lost = rng.random(n) < 0.01
    lost[n // 2] = True      # (one at least, however few pairs)
    out = [payload[:first]]
    for i in np.argsort(where, kind="stable"):
        if lost[i // 2] and i % 2 == (i // 2) % 2:
            continue
        out.append(recs[i][1])
        if rng.random() < 0.03:
            copy = bytearray(recs[i][1])
            struct.pack_into("<H", copy, 18, struct.unpack_from("<H", copy, 18)[0] | 0x800)
            out.append(bytes(copy))
    return b"".join(out)


def no_pair_prefix(payload, first, n_first):
    """S with the first mates of its first n_first pairs in front of everything else: the chunks that lie inside that prefix complete no pair"""
    recs, _, _ = tbi.split_records(payload, first)
    w = walk(payload, first)
    head = [w["order"][2 * k] for k in range(min(n_first, w["pairs"]))]
    taken = set(head)
    return payload[:first] + b"".join(recs[i][1] for i in head) + b"".join(r for i, (_, r) in enumerate(recs) if i not in taken)


def drain_stats(path, lib, device, collate, **kw):
    fe = api.BamFrontEnd(path, device=device, lib=lib, collate_mem=(1 << 30) if collate else None, **kw)
    n, got = tbi.drain(fe, False)
    st = fe.stats()
    fe.close()
    return n, got, st


def check_front_end(lib, S, first, tmp, tag, configs, device=0, modes=(0, 1, 2), max_len=160, min_peak=0):
    """configs: (batch_pairs, chunk_pairs, the chunks the stream must take at least)"""
    w = walk(S, first)
    assert w["bad"] is None and w["paired"]
    paths = {}
    for k, pay in (("S", S), ("C", w["C"])):
        paths[k] = os.path.join(tmp, "%s_%s.bam" % (tag, k))
        open(paths[k], "wb").write(tbi.bgzf(pay))
    for batch, chunk, least in configs:
        for mode in modes:
            kw = dict(batch_pairs=batch, chunk_pairs=chunk, slot_mode=mode, max_read_len=max_len)
            n_want, want, _ = drain_stats(paths["C"], lib, device, False, **kw)
            assert n_want == w["pairs"]
            for k in ("S", "C"):      # (on C itself the flag gives the same batches as no flag)
                n_got, got, st = drain_stats(paths[k], lib, device, True, **kw)
                what = (tag, k, batch, chunk, mode)
                assert n_got == n_want and st["chunks"] >= least, (what, n_got, n_want, st["chunks"])
                assert st["bam_orphans"] == (len(w["orphans"]) if k == "S" else 0) and st["bam_records"] == (w["records"] if k == "S" else 2 * w["pairs"]), what
                assert st["bam_skipped"] == (w["records"] - w["kept"] if k == "S" else 0), what
                if k == "S":
                    assert st["bam_held_peak_records"] >= max(min_peak, len(w["orphans"])) and st["ms_bam_collate"] >= 0, what
                for e in range(2):
                    for j in range(3):
                        assert got[e][j].shape == want[e][j].shape and (got[e][j] == want[e][j]).all(), (what, e, ("heads", "lengths", "names")[j])


def check_front_end_seeded(lib, tmp, device=0):
    pay, first = seeded_stream()
    check_front_end(lib, pay, first, tmp, "seeded", [(250, 4000, 1)], device=device)
    # megabytes of payload, so that its chunks are chunks of payload: three chunks, many chunks; then the same behind 20,000 first mates -- 4.6 MB, more than
    # the first chunks hold, so they complete no pair and the stream goes on
    big, first = seeded_stream(24000, seed=7)
    check_front_end(lib, big, first, tmp, "big", [(500, 12000, 3), (500, 2000, 6)], device=device, modes=(0,))
    # (six chunks or more, the first ones the shortest, over 10 MB: the first chunk ends inside the prefix.  What waits is counted at the chunks' ends, so the peak
    #  is not the prefix's 20,000 to the record -- half of them waiting at once is more than any chunk of this stream could leave without the prefix)
    check_front_end(lib, no_pair_prefix(big, first, 20000), first, tmp, "prefix", [(500, 2000, 6)], device=device, modes=(1,), min_peak=10000)


def check_front_end_golden(lib, g, tmp, device=0):
    pay, first, max_len = tbi.golden_bam(g)
    max_len = max(max_len, (max(len(s) for _, s, _ in tbi.fastq_records(g["fq2"])) + 15) // 16 * 16)
    batch = g["batch"]
    check_front_end(lib, shuffle_like_the_seeded_stream(pay, first), first, tmp, "qc", [(batch, max(batch, g["n_pairs"] // 3 // batch * batch), 1)], device=device, max_len=max_len)


def test_front_end_batches_of_the_seeded_stream_equal_those_of_its_collated_file(emu_lib, tmp_path):
    check_front_end_seeded(emu_lib, str(tmp_path))


def test_front_end_batches_of_a_shuffled_golden_equal_those_of_its_collated_file(golden_cases, emu_lib, tmp_path):
    check_front_end_golden(emu_lib, golden_cases["qc"], str(tmp_path))


def test_front_end_refusal_and_bound_name_the_record(emu_lib, tmp_path):
    hdr = tbi.bam_header()
    for k, (what, pay, bad) in enumerate(refusal_cases()):
        path = str(tmp_path / ("bad%d.bam" % k))
        open(path, "wb").write(tbi.bgzf(hdr + pay, member=120))
        fe = api.BamFrontEnd(path, batch_pairs=2, chunk_pairs=4, lib=emu_lib, collate_mem=1 << 20)
        with pytest.raises(api.FastquickError) as ei:
            tbi.drain(fe, False)
        fe.close()
        assert "BAM record %d:" % bad[0] in str(ei.value), (what, str(ei.value))
        if bad[1] == "dup":
            assert "a second record of this name and side before the mate of the first" in str(ei.value), (what, str(ei.value))
    pay, _ = seeded_stream()
    path = str(tmp_path / "seeded.bam")
    open(path, "wb").write(tbi.bgzf(pay))
    fe = api.BamFrontEnd(path, batch_pairs=250, chunk_pairs=4000, lib=emu_lib, collate_mem=4096)
    with pytest.raises(api.FastquickError) as ei:
        tbi.drain(fe, False)
    fe.close()
    assert "failed: -5" in str(ei.value) and "--collate_mem 4096" in str(ei.value) and "BAM record 0:" in str(ei.value), str(ei.value)


# ---- 3. the command line ------------------------------------------------------------------------------------------------------------------------
def check_cli_pair(exe, g, tmp, tag, S_path, C_path, timeout=None, sorted_too=True, qc_too=True):
    """--bam_in S --collate against --bam_in C: SAM text, QC files, BAM payload, sorted BAM and index, byte for byte.  Returns the stderr of the collating run."""
    ins = (("_c", ["--bam_in", C_path]), ("_s", ["--bam_in", S_path, "--collate"]))
    sam = [tbi.run_cli(exe, g, os.path.join(tmp, tag + k), inp, "--sam_out", timeout=timeout) for k, inp in ins]
    assert sam[0].stdout == sam[1].stdout and any(ln and not ln.startswith(b"@") for ln in sam[0].stdout.split(b"\n")), tag
    if qc_too:
        n_qc = 0
        for name in tbi.QC_FILES:
            fa, fb = (os.path.join(tmp, tag + k + "." + name) for k, _ in ins)
            a, b = open(fa, "rb").read(), open(fb, "rb").read()
            if name == "FASTQ.csv":      # (it names the input file: as check_cli_equality treats it)
                a = a.replace(os.path.basename(C_path).encode(), os.path.basename(S_path).encode())
            assert a == b, (tag, name)
            n_qc += 1
        assert n_qc == 13
    for k, inp in ins:
        tbi.run_cli(exe, g, os.path.join(tmp, tag + "_u" + k), inp, timeout=timeout)
        if sorted_too:
            tbi.run_cli(exe, g, os.path.join(tmp, tag + "_o" + k), inp, "--sorted_bam", timeout=timeout)
    assert tbi.bgzf_payload(os.path.join(tmp, tag + "_u_c.bam")) == tbi.bgzf_payload(os.path.join(tmp, tag + "_u_s.bam")), tag
    if sorted_too:
        assert tbi.bgzf_payload(os.path.join(tmp, tag + "_o_c.sorted.bam")) == tbi.bgzf_payload(os.path.join(tmp, tag + "_o_s.sorted.bam")), tag
        assert open(os.path.join(tmp, tag + "_o_c.sorted.bam.bai"), "rb").read() == open(os.path.join(tmp, tag + "_o_s.sorted.bam.bai"), "rb").read(), tag
    return sam[1].stderr


def write_S_and_C(S, tmp, tag):
    first, _ = tbi.bam_first_record(S)
    w = walk(S, first)
    assert w["bad"] is None and w["paired"] and w["pairs"]
    paths = []
    for k, pay in (("S", S), ("C", w["C"])):
        paths.append(os.path.join(tmp, "%s_%s.bam" % (tag, k)))
        open(paths[-1], "wb").write(tbi.bgzf(pay))
    return paths[0], paths[1], w


def check_cli_golden(exe, g, tmp, timeout=None, sorted_too=True):
    pay, first, _ = tbi.golden_bam(g)
    S, C, w = write_S_and_C(shuffle_like_the_seeded_stream(pay, first), tmp, "shuf")
    err = check_cli_pair(exe, g, tmp, "shuf", S, C, timeout=timeout, sorted_too=sorted_too)
    assert len(w["orphans"]) > 0 and err.count(b"WARNING - BAM input: %d records without a mate" % len(w["orphans"])) == 1, err.decode(errors="replace")[-2000:]
    return S, C


def check_cli_round_trip(exe, g, tmp, timeout=None):
    """the O.sorted.bam this program writes for the golden, fed back with --bam_in --collate: equal to the run on C built from that file's records by the walk"""
    tbi.run_cli(exe, g, os.path.join(tmp, "rt"), ["--fastq_1", g["fq1"], "--fastq_2", g["fq2"]], "--sorted_bam", timeout=timeout)
    srt = os.path.join(tmp, "rt.sorted.bam")
    S, C, w = write_S_and_C(tbi.bgzf_payload(srt), tmp, "fed")
    assert S and any(b - a != 1 for a, b in zip(w["order"][0::2], w["order"][1::2])), "the sorted file's mates are not all adjacent"
    check_cli_pair(exe, g, tmp, "fed", srt, C, timeout=timeout, sorted_too=False, qc_too=False)


def test_command_line_collate_equals_the_run_on_the_collated_file(golden_cases, emu_cli, tmp_path):
    g = golden_cases["qc"]
    S, C = check_cli_golden(emu_cli, g, str(tmp_path))
    # without the flag the file is still refused, with today's message
    run = tbi.run_cli(emu_cli, g, str(tmp_path / "r"), ["--bam_in", S], ok=False)
    assert run.returncode != 0 and b"mates are not adjacent: collate the file by name first" in run.stderr and not run.stdout
    for inputs, extra, word in ((["--fastq_1", g["fq1"], "--fastq_2", g["fq2"]], ["--collate"], b"--collate"), (["--bam_in", C], ["--collate_mem", "1000000"], b"--collate_mem"),
                                (["--bam_in", S], ["--collate", "--host_reader"], b"--host_reader"), (["--bam_in", S], ["--collate", "--frac_samp", "0.5"], b"--frac_samp")):
        run = tbi.run_cli(emu_cli, g, str(tmp_path / "r"), inputs, *extra, ok=False)
        assert run.returncode != 0 and word in run.stderr and not run.stdout, extra
    run = tbi.run_cli(emu_cli, g, str(tmp_path / "r"), ["--bam_in", S], "--collate", "--collate_mem", "2000", ok=False)
    assert run.returncode != 0 and b"--collate_mem 2000" in run.stderr


def test_command_line_round_trip_of_its_own_sorted_bam(golden_cases, emu_cli, tmp_path):
    check_cli_round_trip(emu_cli, golden_cases["qc"], str(tmp_path))


# ---- 4. the host code under AddressSanitizer / UBSan: a program of its own --------------------------------------------------------------------
def write_check_corpus(path):
    """the kernel-entry corpus and the seeded stream with the walk's results, as the check program reads it"""
    cases = [(p, f, n) for _, p, f, n in good_cases()] + [(p, 0, 1) for _, p, _ in refusal_cases()] + [seeded_stream() + (1,)]
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for pay, first, n_ref in cases:
            w = walk(pay, first)
            t = tbi.transcode(w["C"], first) if not w["bad"] else dict(text1=b"", text2=b"")
            bad = w["bad"] or (-1, None)
            t1, t2 = t["text1"] or b"", t["text2"] or b""
            fh.write(struct.pack("<iqq", n_ref, first, len(pay)) + pay)
            fh.write(struct.pack("<qiqqqq", bad[0], KIND_RANK.get(bad[1], 0), w["pairs"], len(w["orphans"]) if w["paired"] else 0, len(t1), len(t2)) + t1 + t2)
    return len(cases)


def test_host_code_under_sanitizers(tmp_path):
    subprocess.check_call(["make", "-s", "-C", CHECK_DIR, "bam_collate_check"])
    corpus = str(tmp_path / "corpus.bin")
    n_cases = write_check_corpus(corpus)
    pay, first = seeded_stream(24000, seed=7)
    w = walk(pay, first)
    bam = str(tmp_path / "stream.bam")
    open(bam, "wb").write(tbi.bgzf(pay))
    run = subprocess.run([os.path.join(CHECK_DIR, "bam_collate_check"), corpus, bam, "500", "2000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    assert b"ok: %d cases, %d pairs, %d orphans" % (n_cases, w["pairs"], len(w["orphans"])) in run.stdout, run.stdout


# ---- 5. GPU tier: every check a process of its own under a time limit ---------------------------------------------------------------------------
def gpu_step(*args, env=None):
    run = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=tbi.GPU_STEP_SEC, env=dict(os.environ, **(env or {})))
    assert run.returncode == 0, (run.stdout.decode(errors="replace")[-1500:], run.stderr.decode(errors="replace")[-3000:])
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [None, "0"])
def test_kernel_entry_on_the_gpu(bits):
    env = {k: v for k, v in os.environ.items() if k != "FASTQUICK_BAM_HASH_BITS"}
    if bits is not None:
        env["FASTQUICK_BAM_HASH_BITS"] = bits
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "entry"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=tbi.GPU_STEP_SEC, env=env)
    assert run.returncode == 0, (run.stdout.decode(errors="replace")[-1500:], run.stderr.decode(errors="replace")[-3000:])


@pytest.mark.gpu
def test_front_end_on_the_gpu(golden_cases, tmp_path):
    gpu_step("frontend", golden_cases["qc"]["dir"], "qc", str(tmp_path))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["qc", "wide"])
def test_command_line_on_the_gpu(tag, golden_cases, tmp_path):
    check_cli_golden(tbi.CLI_GPU, golden_cases[tag], str(tmp_path), timeout=tbi.GPU_STEP_SEC, sorted_too=tag == "qc")


@pytest.mark.gpu
def test_command_line_round_trip_on_the_gpu(golden_cases, tmp_path):
    check_cli_round_trip(tbi.CLI_GPU, golden_cases["qc"], str(tmp_path), timeout=tbi.GPU_STEP_SEC)


if __name__ == "__main__":
    lib = api.load_library()
    what = sys.argv[1]
    if what == "entry":
        check_entry_corpus(lib)
        check_collate_mem(lib)
    elif what == "frontend":
        g = golden_util.case_params(sys.argv[3])
        d = sys.argv[2]
        g.update(dir=d, fq1=os.path.join(d, "reads_1.fq"), fq2=os.path.join(d, "reads_2.fq"))
        check_front_end_golden(lib, g, sys.argv[4])
    else:
        raise SystemExit("unknown check " + what)
    print("ok")
