"""BAM input by read group and with original qualities (`align --bam_in X.bam --bam_rg ID... --bam_oq`; DESIGN.md 5d''): the walk of the auxiliary
fields on the device (fq_bamin.h (b'')).  The yardstick is Python throughout: a serial walk of every record's auxiliary fields (SAM specification 4.2.4),
the selection, then the existing transcoder (tests/test_bam_input.py) and the existing walk of the collation (tests/test_bam_collate.py) on X_sel -- the file
that holds X's header and, in X's order, its skipped and its selected records; with --bam_oq a copy of record_text with the OQ rule says the text, and X_sel with that rule's qualities written into QUAL carries it to them.
Host-loop tier here; the GPU tier runs the same checks, each a process of its own."""
from __future__ import annotations

import heapq
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import golden_util  # noqa: E402
import test_bam_collate as tbc  # noqa: E402
import test_bam_input as tbi  # noqa: E402
from fastquick_amd import api  # noqa: E402

CHECK_DIR = os.path.join(ROOT, "tests", "bam_tags_check")
KIND_RANK = dict(tbc.KIND_RANK, aux=8, oq=9)
SIZE = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}
WANTED = (b"lane1", b"lane2")
MEMBER = 300


@pytest.fixture(scope="module")
def emu_lib():
    subprocess.check_call(["make", "-s", "-C", tbi.EMU_DIR, "libfq_emu.so"])
    return api.load_library(os.path.join(tbi.EMU_DIR, "libfq_emu.so"))


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------------
def aux_walk(r: bytes):
    """(good, the first RG:Z value or None, the first OQ:Z value or None) of a whole record; where the walk fails, what it found up to there"""
    f = tbi.fields(r)
    found = {}

    def walk():
        p, end = 36 + f["l_name"] + 4 * f["n_cig"] + (f["l_seq"] + 1) // 2 + f["l_seq"], 4 + f["bs"]
        if p > end:
            return False
        while p < end:
            if p + 3 > end:
                return False
            tag, ty = r[p:p + 2], r[p + 2]
            first = tag in (b"RG", b"OQ") and tag not in found
            if first and ty != ord("Z"):
                return False
            p += 3
            if ty in (ord("Z"), ord("H")):
                q = r.find(b"\0", p, end)
                if q < 0:
                    return False
                if first:
                    found[tag] = r[p:q]
                p = q + 1
            elif ty == ord("B"):
                if p + 5 > end or r[p] == ord("A") or r[p] not in SIZE:
                    return False
                p += 5 + SIZE[r[p]] * struct.unpack_from("<I", r, p + 1)[0]
            elif ty in SIZE:
                p += SIZE[ty]
            else:
                return False
            if p > end:
                return False
        return True
    good = walk()
    return good, found.get(b"RG"), found.get(b"OQ")


def record_text_oq(r: bytes) -> bytes:
    """a copy of tests/test_bam_input.py's record_text with the one line changed: a record that has OQ:Z prints those bytes as its quality line"""
    f = tbi.fields(r)
    nm = r[36:36 + f["l_name"] - 1]
    at = 36 + f["l_name"] + 4 * f["n_cig"]
    l = f["l_seq"]
    packed, qual = r[at:at + (l + 1) // 2], r[at + (l + 1) // 2:at + (l + 1) // 2 + l]
    codes = [(packed[i >> 1] >> (0 if i & 1 else 4)) & 15 for i in range(l)]
    good, _, oq = aux_walk(r)
    q = oq if good and oq is not None else bytes(min(v + 33, 126) for v in qual)
    if f["flag"] & 0x10:
        seq = bytes(tbi.COMPLEMENT[c] for c in reversed(codes))
        q = q[::-1]
    else:
        seq = bytes(tbi.LETTERS[c] for c in codes)
    return b"@" + nm + b"\n" + seq + b"\n+\n" + q + b"\n"


def oq_fits(r: bytes, q) -> bool:
    return q is not None and len(q) == tbi.fields(r)["l_seq"] and all(0x21 <= b <= 0x7e for b in q)


def oq_as_qual(payload: bytes, first: int) -> bytes:
    """The payload whose text under the plain rule is this payload's text under the OQ rule: every walked record whose OQ fits gets QUAL := OQ - 33 (0..93, so
    min(q + 33, 126) gives the OQ byte back); nothing moves.  This is how the transcoder, the collation walk and the FASTQ front end of the existing tests --
    none of which knows OQ -- serve as the reference under --bam_oq; record_text_oq above says the rule itself, and the two are held to each other below."""
    recs, chain_end, _ = tbi.split_records(payload, first)
    out = [payload[:first]]
    for _, r in recs:
        good, _, q = aux_walk(r)
        if not tbi.fields(r)["flag"] & 0x900 and good and oq_fits(r, q):
            f = tbi.fields(r)
            at = 36 + f["l_name"] + 4 * f["n_cig"] + (f["l_seq"] + 1) // 2
            r = r[:at] + bytes(b - 33 for b in q) + r[at + f["l_seq"]:]
        out.append(r)
    return b"".join(out) + payload[chain_end:]


def select(payload: bytes, first: int, ids=(), oq=False) -> dict:
    """X_sel (header, then X's skipped and selected records in X's order, then what X's chain leaves over), the X ordinals and offsets of its records, the
    refusals of kinds 8 / 9 by X ordinal, and the counts"""
    recs, chain_end, end_flag = tbi.split_records(payload, first)
    keep, tag_bad, unselected, with_oq = [], [], 0, set()
    for i, (_, r) in enumerate(recs):
        if tbi.fields(r)["flag"] & 0x900:
            keep.append(i)
            continue
        good, rg, q = aux_walk(r)
        if not good:
            tag_bad.append((i, "aux"))      # (selected or not says the RG the walk met in front of what stopped it)
        if ids and rg not in ids:
            unselected += 1
            continue
        keep.append(i)
        if good and oq and q is not None:
            if not oq_fits(r, q):
                tag_bad.append((i, "oq"))
            else:
                with_oq.add(i)
    X_sel = payload[:first] + b"".join(recs[i][1] for i in keep) + payload[chain_end:]
    return dict(X_sel=X_sel, ords=keep, offs=[recs[i][0] for i in keep], tag_bad=tag_bad, unselected=unselected, with_oq=with_oq, records=len(recs), chain_end=chain_end, end_flag=end_flag)


def first_bad(bads):
    return min(bads, key=lambda x: (x[0], KIND_RANK[x[1]])) if bads else None


def want_transcode(payload, first, ids, oq):
    """the contract on X under the options, in X's ordinals and offsets"""
    s = select(payload, first, ids, oq)
    t = tbi.transcode(oq_as_qual(s["X_sel"], first) if oq else s["X_sel"], first)
    n_sel = len(s["ords"])
    used = s["ords"][t["used_records"]] if t["used_records"] < n_sel else s["records"]
    carry = s["offs"][t["used_records"]] if t["used_records"] < n_sel else s["chain_end"]
    bads = [b for b in s["tag_bad"] if b[0] < used] + ([(s["ords"][t["bad"][0]], t["bad"][1])] if t["bad"] else [])
    bad = first_bad(bads)
    return dict(t, records=s["records"], used_records=used, carry_from=carry, chain_end=s["chain_end"], bad=bad, text1=None if bad else t["text1"], text2=None if bad else t["text2"],
                unselected=len(set(range(used)) - set(s["ords"])), oq_records=sum(1 for i in s["with_oq"] if i < used), sel=s)


def check_entry(lib, payload, cuts, first=0, n_ref=1, ids=(), oq=False, device=0, what=""):
    want = want_transcode(payload, first, ids, oq)
    got = api.bam_transcode_device(payload, cuts, n_ref, first, device=device, lib=lib, rg=ids, oq=oq)
    for k in ("records", "kept", "units", "used_records", "chain_end", "end_flag", "carry_from"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    if want["bad"]:
        assert (got["bad_record"], got["bad_kind"]) == want["bad"], (what, got["bad_record"], got["bad_kind"], want["bad"])
    else:
        assert got["bad_record"] == -1, (what, got["bad_record"], got["bad_kind"])
        assert got["text1"] == want["text1"] and got["text2"] == want["text2"], what
        assert got["unselected"] == want["unselected"] and got["oq_records"] == want["oq_records"], (what, got["unselected"], want["unselected"], got["oq_records"], want["oq_records"])
    return got, want


def check_collate(lib, payload, first=0, n_ref=1, ids=(), oq=False, per_chunk=0, device=0, what=""):
    s = select(payload, first, ids, oq)
    w = tbc.walk(s["X_sel"], first)
    cuts = list(range(0, len(payload), MEMBER))
    got = api.bam_collate_device(payload, cuts, n_ref, first, members_per_chunk=per_chunk, device=device, lib=lib, rg=ids, oq=oq)
    bad = first_bad(s["tag_bad"] + ([(s["ords"][w["bad"][0]], w["bad"][1])] if w["bad"] else []))
    tag = (what, per_chunk, os.environ.get("FASTQUICK_BAM_HASH_BITS"))
    if bad:
        assert (got["bad_record"], got["bad_kind"]) == bad, (tag, got["bad_record"], got["bad_kind"], bad)
        return got, w
    t = tbi.transcode(oq_as_qual(w["C"], first) if oq else w["C"], first)
    assert t["bad"] is None and got["bad_record"] == -1, (tag, got["bad_record"], got["bad_kind"])
    assert got["records"] == s["records"] and got["kept"] == w["kept"] and got["pairs"] == w["pairs"], tag
    assert not w["paired"] or got["orphans"] == len(w["orphans"]), (tag, got["orphans"], len(w["orphans"]))
    assert got["text1"] == t["text1"] and got["text2"] == (t["text2"] or b""), tag
    assert got["unselected"] == s["unselected"], (tag, got["unselected"], s["unselected"])
    if w["paired"]:
        orphans = {s["ords"][i] for i in w["orphans"]}
        assert got["oq_records"] == len(s["with_oq"] - orphans), (tag, got["oq_records"])
    return got, w


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------------
def Z(tag: bytes, val: bytes) -> bytes:
    return tag + b"Z" + val + b"\0"


def B(tag: bytes, sub: bytes, vals) -> bytes:
    fmt = {b"c": "b", b"C": "B", b"s": "h", b"S": "H", b"i": "i", b"I": "I", b"f": "f"}[sub]
    return tag + b"B" + sub + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), fmt), *vals)


EVERY_TYPE = (b"XAAq" + b"Xcc\xff" + b"XCC\x07" + b"Xss" + struct.pack("<h", -2) + b"XSS" + struct.pack("<H", 65535) + b"Xii" + struct.pack("<i", -3) + b"XII" + struct.pack("<I", 1 << 31) +
              b"Xff" + struct.pack("<f", 1.5) + Z(b"XZ", b"text") + b"XHH1AE3\0" + B(b"Bc", b"c", [-1, 2]) + B(b"BC", b"C", [1, 2, 3]) + B(b"Bs", b"s", [-5]) + B(b"BS", b"S", [5, 6]) +
              B(b"Bi", b"i", [-7, 8, 9]) + B(b"BI", b"I", [7]) + B(b"Bf", b"f", [0.5, 2.0]) + B(b"B0", b"S", []))
L = 20      # bases of the corpus' reads


def pair(rng, name: bytes, tags1: bytes, tags2: bytes = None, l=L, rev=False, quals=None):
    """the two mates of a pair, adjacent, each with its own auxiliary fields"""
    out = []
    for side, tg in ((0x41, tags1), (0x81, tags1 if tags2 is None else tags2)):
        c, q = tbi.rand_read(rng, l)
        out.append(tbi.bam_record(name, side | (0x10 if rev else 0), c, q if quals is None else quals, tags=tg))
    return out


def OQ(rng, l=L) -> bytes:
    return Z(b"OQ", bytes(rng.integers(0x21, 0x7f, l).tolist()))


def good_records(rng):
    """(what, records): pairs with adjacent mates; WANTED selects some of them"""
    rg1, rg2 = Z(b"RG", b"lane1"), Z(b"RG", b"lane2")
    spell = b"RGZlane1\0"
    cases = [("every type and subtype, RG last", pair(rng, b"types", EVERY_TYPE + rg1)),
             ("RG first", pair(rng, b"first", rg1 + EVERY_TYPE)),
             ("RG between", pair(rng, b"mid", b"NMC\x01" + rg1 + Z(b"PG", b"bwa"))),
             ("RG absent", pair(rng, b"absent", b"NMC\x01" + Z(b"PG", b"bwa"))),
             ("RG twice: the first decides (wanted)", pair(rng, b"twiceA", rg1 + Z(b"RG", b"other"))),
             ("RG twice: the first decides (not wanted)", pair(rng, b"twiceB", Z(b"RG", b"other") + rg1)),
             ("an ID that is a proper prefix of a wanted one", pair(rng, b"prefix", Z(b"RG", b"lane"))),
             ("an ID of which a wanted one is a proper prefix", pair(rng, b"longer", Z(b"RG", b"lane10"))),
             ("an empty ID", pair(rng, b"empty", Z(b"RG", b""))),
             ("the second wanted ID", pair(rng, b"second", rg2 + b"NMC\x00")),
             ("decoy: XX:Z:RGZlane1", pair(rng, b"decoyZ", Z(b"XX", b"RGZlane1"))),
             ("decoy: a B:C array that spells RGZlane1", pair(rng, b"decoyB", B(b"XB", b"C", list(spell)))),
             ("decoy: a B:C array that spells it, behind the real group", pair(rng, b"decoyC", Z(b"RG", b"other") + B(b"XB", b"C", list(spell)))),
             ("decoy: OQ bytes inside an H value", pair(rng, b"decoyH", rg1 + b"XHH" + b"OQZ" + b"I" * L + b"\0")),
             ("an aux area of length 0", pair(rng, b"noaux", b"")),
             ("an aux area that ends with the record: a Z's NUL is its last byte", pair(rng, b"ends", b"NMC\x02" + rg1)),
             ("OQ on both mates", pair(rng, b"oq", rg1 + OQ(rng), OQ(rng) + rg1)),
             ("OQ on a reverse-strand record", pair(rng, b"oqrev", rg2 + OQ(rng), rev=True)),
             ("OQ beside QUAL 0xff", pair(rng, b"oqff", rg1 + OQ(rng), quals=[255] * L)),
             ("OQ on one mate only", pair(rng, b"oqone", rg1 + OQ(rng), rg1)),
             ("OQ twice: the first decides", pair(rng, b"oqtwice", rg1 + OQ(rng) + Z(b"OQ", b"short"))),
             ("OQ at the caps 0x21 and 0x7e", pair(rng, b"oqcap", rg1 + Z(b"OQ", b"!~" * (L // 2)))),
             ("OQ on a record that is not selected", pair(rng, b"oqother", Z(b"RG", b"other") + Z(b"OQ", b"bad length"))),
             ("an odd read with OQ, reversed", pair(rng, b"odd", rg1 + OQ(rng, 17), l=17, rev=True))]
    return cases


def good_payload(seed=20261020, for_all=False):
    """for_all: without the pair whose OQ only a selection keeps from being checked"""
    rng = np.random.default_rng(seed)
    recs = [r for what, rs in good_records(rng) for r in rs if not (for_all and what == "OQ on a record that is not selected")]
    sec = tbi.bam_record(b"sec", 0x141, [1] * 9, [30] * 9, tags=b"XX")      # (a skipped record is not walked: its two stray bytes refuse nothing)
    sup = tbi.bam_record(b"sup", 0x881, [2] * 5, [30] * 5, tags=Z(b"RG", b"lane1"))
    return b"".join([sec] + recs[:7] + [sup] + recs[7:] + [sec])


def bad_aux_fields():
    """(what, bytes that no walk gets through)"""
    return [("an unknown type", b"XQQ\x01"), ("an unknown B subtype", b"XBBx" + struct.pack("<I", 1) + b"\0"), ("a B subtype A", b"XBBA" + struct.pack("<I", 1) + b"\0"),
            ("a value that runs beyond the area", b"Xii\x01\x02"), ("a B whose count runs beyond the area", B(b"XB", b"i", [1, 2])[:-1]),
            ("a B whose count x size overflows 32 bits", b"XBBI" + struct.pack("<I", 0x40000001) + b"\0" * 4), ("a B cut inside its count", b"XBBc\x01\x00"),
            ("a Z without NUL", b"XZZnonul"), ("an H without NUL", b"XHH1A"), ("one stray byte", b"X"), ("two stray bytes", b"XY")]


def refusal_cases():
    """(what, payload, ids, oq, (ordinal, kind))"""
    rng = np.random.default_rng(41)
    rg1, other = Z(b"RG", b"lane1"), Z(b"RG", b"other")
    ok = pair(rng, b"ok", rg1)
    out = []
    for what, junk in bad_aux_fields():
        out.append((what + ", on a selected record", b"".join(ok + pair(rng, b"bad", rg1 + junk, rg1)), WANTED, False, (2, "aux")))
        out.append((what + ", on a record of another group", b"".join(ok + pair(rng, b"bad", other, other + junk) + ok), WANTED, False, (3, "aux")))
        out.append((what + ", with --bam_oq alone", b"".join(ok + ok + pair(rng, b"bad", junk)), (), True, (4, "aux")))
    out.append(("RG of type A", b"".join(ok + pair(rng, b"bad", b"RGAx" + rg1)), WANTED, False, (2, "aux")))
    out.append(("RG of type H on a record without another", b"".join(pair(rng, b"bad", b"RGHlane1\0")), WANTED, False, (0, "aux")))
    out.append(("a second RG of another type is a field like any other", b"".join(pair(rng, b"fine", rg1 + b"RGAx") + pair(rng, b"bad", rg1 + b"OQAx")), WANTED, False, (2, "aux")))
    out.append(("OQ of type H, without --bam_oq", b"".join(ok + pair(rng, b"bad", rg1 + b"OQH2121\0")), WANTED, False, (2, "aux")))
    out.append(("OQ one byte short", b"".join(ok + pair(rng, b"bad", rg1, rg1 + Z(b"OQ", b"I" * (L - 1)))), WANTED, True, (3, "oq")))
    out.append(("OQ one byte long", b"".join(ok + pair(rng, b"bad", rg1 + Z(b"OQ", b"I" * (L + 1)))), (), True, (2, "oq")))
    out.append(("OQ empty", b"".join(ok + pair(rng, b"bad", Z(b"OQ", b"") + rg1)), WANTED, True, (2, "oq")))
    out.append(("OQ with a space", b"".join(ok + pair(rng, b"bad", rg1 + Z(b"OQ", b"I" * 5 + b" " + b"I" * (L - 6)))), WANTED, True, (2, "oq")))
    out.append(("OQ with 0x7f", b"".join(pair(rng, b"bad", rg1, rg1 + Z(b"OQ", b"I" * (L - 1) + b"\x7f"))), WANTED, True, (1, "oq")))
    out.append(("OQ that does not fit, on a record of another group: not checked", b"".join(pair(rng, b"fine", other + Z(b"OQ", b"x")) + ok + pair(rng, b"bad", rg1 + Z(b"OQ", b"x"))), WANTED, True,
                (4, "oq")))
    single = tbi.bam_record(b"bad", 0x4, *tbi.rand_read(rng, L), tags=rg1 + b"X")
    out.append(("a record refused for kinds 1 and 8 reports 1", b"".join(ok + [single] + ok), WANTED, False, (2, "mixed")))
    out.append(("kinds 8 and 2 on one record: 2", b"".join(ok + [tbi.bam_record(b"bad", 0x41, [], [], tags=rg1 + b"X")] + ok), WANTED, False, (2, "l_seq0")))
    out.append(("mates of different groups, adjacent: the selected one meets the next record", b"".join(ok + pair(rng, b"split", rg1, other) + pair(rng, b"next", rg1)), WANTED, False, (2, "mates")))
    out.append(("an earlier refusal of the pairing wins over a later walk", b"".join(ok + pair(rng, b"p", rg1)[:1] + pair(rng, b"q", rg1)[1:] + pair(rng, b"bad", rg1 + b"X")), WANTED, False, (2, "names")))
    return out


def cuts_for(payload, member):
    return list(range(0, len(payload), member)) if member else [0]


def check_entry_corpus(lib, device=0):
    pay, pay_all = good_payload(), good_payload(for_all=True)
    hdr = tbi.bam_header((("1", 1000), ("2", 500)))
    for member in (0, MEMBER):
        for ids, oq in ((WANTED, False), ((), True), (WANTED, True), ((b"lane2",), True), ((b"nobody",), False)):
            x = pay if ids else pay_all
            got, want = check_entry(lib, x, cuts_for(x, member), ids=ids, oq=oq, device=device, what=("good", member, ids, oq))
            assert want["bad"] is None, (ids, oq, want["bad"])
            if ids == WANTED:
                assert want["units"] == 14 and want["unselected"] == 20, (want["units"], want["unselected"])
            if oq and not ids:
                assert want["units"] == 23 and want["oq_records"] == 13, (want["units"], want["oq_records"])
        got, _ = check_entry(lib, hdr + pay, cuts_for(hdr + pay, member), first=len(hdr), n_ref=2, ids=WANTED, oq=True, device=device, what=("behind a header", member))
        # (the payload cut inside the last pair: its first mate is carried, and what the walk says of it is said with the next payload)
        cut = pay[:len(pay) - 70]
        check_entry(lib, cut, cuts_for(cut, member), ids=WANTED, oq=True, device=device, what=("cut", member))
        for what, p, ids, oq, bad in refusal_cases():
            got, want = check_entry(lib, p, cuts_for(p, member), ids=ids, oq=oq, device=device, what=(what, member))
            assert want["bad"] == bad, (what, want["bad"], bad)      # (the yardstick itself against the case's statement)
            assert got["text1"] is None, what
    # a walk that fails on a last record without its mate: the record is carried, and what the walk says of it is said with the next payload
    rng = np.random.default_rng(3)
    p = b"".join(pair(rng, b"ok", Z(b"RG", b"lane1")) + pair(rng, b"bad", Z(b"RG", b"lane1") + b"X")[:1])
    got, want = check_entry(lib, p, [0], ids=WANTED, device=device, what="carried")
    assert want["bad"] is None and got["used_records"] == 2 and got["units"] == 1


def collate_payloads():
    """(what, payload, ids, oq): mates apart, so that records are held -- with their OQ -- from chunk to chunk; mates of different groups become orphans"""
    rng = np.random.default_rng(43)
    rg1, rg2, other = Z(b"RG", b"lane1"), Z(b"RG", b"lane2"), Z(b"RG", b"other")
    firsts, seconds = [], []
    for k in range(12):
        tg = (rg1, rg2, other)[k % 3]
        a, b = pair(rng, b"far%d" % k, tg + (OQ(rng, 40) if k % 2 else b""), (OQ(rng, 40) if k % 4 < 2 else b"") + tg, l=40, rev=k % 5 == 0)
        firsts.append(a if k % 2 else b); seconds.append(b if k % 2 else a)
    split = pair(rng, b"split", rg1 + OQ(rng), other)      # (one mate selected, the other not: an orphan)
    lone = pair(rng, b"lone", rg2 + OQ(rng))[:1]
    # the same names in two groups, as a merged file of two lanes' runs has them: the records of the other group take no part
    twin = pair(rng, b"twin", rg1) + pair(rng, b"twin", other)
    stream = firsts[:6] + split[:1] + twin[:1] + twin[2:3] + firsts[6:] + lone + seconds[:6] + twin[3:] + twin[1:2] + split[1:] + seconds[6:]
    pay = b"".join(stream)
    adjacent = good_payload()
    return [("mates apart", pay, WANTED, True), ("mates apart, no selection", pay, (), True), ("mates apart, no OQ", pay, (b"lane1",), False), ("adjacent", adjacent, WANTED, True)]


def check_collate_corpus(lib, device=0):
    for per in (0, 1):
        for what, pay, ids, oq in collate_payloads():
            got, w = check_collate(lib, pay, ids=ids, oq=oq, per_chunk=per, device=device, what=what)
            if what == "mates apart":
                assert len(w["orphans"]) == 2 and got["pairs"] == 9, (len(w["orphans"]), got["pairs"])
                if per:
                    assert got["held_peak_records"] >= 6 and got["chunks"] >= 8
        for what, p, ids, oq, bad in refusal_cases():
            if bad[1] in ("aux", "oq"):
                check_collate(lib, p, ids=ids, oq=oq, per_chunk=per, device=device, what=what)


# ---- 1. the kernel entries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [None, "pieces"])
def test_kernel_entry_against_the_walk_and_the_transcoder(fill, emu_lib, monkeypatch):
    if fill:
        monkeypatch.setenv("FASTQUICK_BAM_FILL", fill)      # (the host-loop library reads it at every call; the HIP library once per process)
    else:
        monkeypatch.delenv("FASTQUICK_BAM_FILL", raising=False)
    check_entry_corpus(emu_lib)


@pytest.mark.parametrize("bits", [None, "0"])
def test_collating_entry_holds_the_offsets_of_oq(bits, emu_lib, monkeypatch):
    if bits is None:
        monkeypatch.delenv("FASTQUICK_BAM_HASH_BITS", raising=False)
    else:
        monkeypatch.setenv("FASTQUICK_BAM_HASH_BITS", bits)
    check_collate_corpus(emu_lib)


def test_the_yardstick_on_plain_cases():
    r = tbi.bam_record(b"n", 0x51, [1, 2, 4, 8], [1, 2, 3, 4], tags=Z(b"RG", b"g") + Z(b"OQ", b"ABCD") + Z(b"RG", b"h"))
    assert aux_walk(r) == (True, b"g", b"ABCD")
    assert record_text_oq(r).endswith(b"+\nDCBA\n") and tbi.record_text(r).endswith(b'+\n%$#"\n')
    # the OQ rule, and the payload that carries it in QUAL: one text, record by record, over the corpus; without OQ the copy is the original
    pay = good_payload(for_all=True)
    recs, _, _ = tbi.split_records(pay, 0)
    as_qual, _, _ = tbi.split_records(oq_as_qual(pay, 0), 0)
    n_oq = 0
    for (_, x), (_, y) in zip(recs, as_qual):
        if tbi.fields(x)["flag"] & 0x900:
            continue
        assert record_text_oq(x) == tbi.record_text(y) and len(x) == len(y)
        assert (record_text_oq(x) == tbi.record_text(x)) == (aux_walk(x)[2] is None or x == y)
        n_oq += x != y
    assert n_oq == 13
    assert aux_walk(tbi.bam_record(b"n", 0x41, [1], [1], tags=Z(b"RG", b"g") + b"XQQ"))[:2] == (False, b"g")
    assert aux_walk(tbi.bam_record(b"n", 0x41, [1], [1], tags=b"X"))[0] is False


# ---- 2. the front end: the batches of X under selection against those of X_sel -------------------------------------------------------------------
def tagged_stream(n_pairs, groups, seed=13, l_seq=100, oq_every=2, single_end_prefix=0, prefix_group=b"other", prefix_pairs=0):
    """an unaligned BAM payload: prefix_pairs pairs of prefix_group (or single_end_prefix single-end records of it), then n_pairs pairs whose groups interleave"""
    rng = np.random.default_rng(seed)
    out = [tbi.bam_header(text="@HD\tVN:1.6\tSO:unsorted\n" + "".join("@RG\tID:%s\tSM:s\n" % g.decode() for g in sorted(set(groups) | {prefix_group})))]
    total = single_end_prefix + 2 * (prefix_pairs + n_pairs)
    codes = np.array([1, 2, 4, 8, 15], dtype=np.uint8)[rng.integers(0, 5, (total, l_seq))]
    quals = rng.integers(2, 41, (total, l_seq), dtype=np.uint8)
    orig = rng.integers(0x21, 0x7f, (total, l_seq), dtype=np.uint8)
    packed = (codes[:, 0::2] << 4 | codes[:, 1::2]).astype(np.uint8)

    def rec(i, nm, fl, grp):
        tags = b"NMC\x01" + Z(b"RG", grp) + (Z(b"OQ", orig[i].tobytes()) if oq_every and i % oq_every == 0 else b"") + B(b"ZB", b"S", [1, 2, 3])
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(nm) + 1, 0, 4680, 0, fl, l_seq, -1, -1, 0) + nm + b"\0" + packed[i].tobytes() + quals[i].tobytes() + tags
        return struct.pack("<I", len(body)) + body
    i = 0
    for k in range(single_end_prefix):
        out.append(rec(i, b"se%07d" % k, 4, prefix_group)); i += 1
    for p in range(prefix_pairs + n_pairs):
        grp = prefix_group if p < prefix_pairs else groups[p % len(groups)]
        for e in range(2):
            out.append(rec(i, b"tg%08d" % p, (0x4d if e == 0 else 0x8d) | (0x10 if i % 5 == 0 else 0), grp)); i += 1
        if p % 97 == 0:
            out.append(tbi.bam_record(b"skipped", 0x901, [1] * 30, [20] * 30))
    return b"".join(out), len(out[0])


def check_front_end(lib, X, first, tmp, tag, ids, oq, batch, chunk, modes=(0, 1, 2), member=65280, least_chunks=1, device=0, max_len=160, least_empty=0):
    """least_empty: so many chunks of X at least hold records and select none of them (fq_frontend_stats_t::bam_empty_chunks)"""
    s = select(X, first, ids, oq)
    assert not s["tag_bad"] and (s["unselected"] > 0 or not ids) and (len(s["with_oq"]) > 0 or not oq)
    X_ref = oq_as_qual(s["X_sel"], first) if oq else s["X_sel"]      # (the reference side knows no OQ)
    paths = {}
    for k, pay in (("X", X), ("ref", X_ref)):
        paths[k] = os.path.join(tmp, "%s_%s.bam" % (tag, k))
        open(paths[k], "wb").write(tbi.bgzf(pay, member=member))
    pr, pr_ref = api.bam_probe(paths["X"], lib=lib, rg=ids, oq=oq), api.bam_probe(paths["ref"], lib=lib)
    for k in ("paired", "first_flag", "first_l_seq", "first_l_name"):
        assert pr[k] == pr_ref[k], (tag, k, pr[k], pr_ref[k])
    se = not pr["paired"]
    for mode in modes:
        kw = dict(batch_pairs=batch, chunk_pairs=chunk, slot_mode=mode, max_read_len=max_len, device=device, lib=lib)
        fe = api.BamFrontEnd(paths["ref"], **kw)
        n_want, want = tbi.drain(fe, se)
        st_ref = fe.stats()
        fe.close()
        fe = api.BamFrontEnd(paths["X"], rg=ids, oq=oq, **kw)
        n_got, got = tbi.drain(fe, se)
        st = fe.stats()
        fe.close()
        what = (tag, mode)
        assert n_got == n_want and n_want > 0 and st["chunks"] >= least_chunks, (what, n_got, n_want, st["chunks"])
        assert st["bam_empty_chunks"] >= least_empty and st_ref["bam_empty_chunks"] == 0, (what, st["bam_empty_chunks"], st["chunks"])
        assert st["bam_records"] == s["records"] and st["bam_unselected"] == s["unselected"] and st["bam_skipped"] == st_ref["bam_skipped"], (what, st["bam_unselected"], s["unselected"])
        assert st["bam_oq_records"] == len(s["with_oq"]) and st_ref["bam_unselected"] == 0 and st_ref["bam_oq_records"] == 0, (what, st["bam_oq_records"], len(s["with_oq"]))
        for e in range(len(want)):
            for j in range(3):
                assert got[e][j].shape == want[e][j].shape and (got[e][j] == want[e][j]).all(), (what, e, ("heads", "lengths", "names")[j])
    return paths


def check_front_end_small(lib, tmp, device=0):
    # members of 300 bytes, records of ~200: the first selected record lies in the third member or behind it
    X, first = tagged_stream(40, (b"lane1", b"other", b"lane2"), prefix_pairs=3)
    s = select(X, first, WANTED)
    assert s["ords"][:2] == [2, 7] and tbi.split_records(X, first)[0][7][0] > 2 * 300      # (ordinal 2 is a skipped record; the first selected one is ordinal 7)
    check_front_end(lib, X, first, tmp, "small", WANTED, True, 4, 8, member=300, device=device)
    # a paired group behind single-end records of another group: the stream is paired
    X, first = tagged_stream(30, (b"lane1", b"lane2", b"other"), single_end_prefix=9)
    paths = check_front_end(lib, X, first, tmp, "behind_se", WANTED, False, 4, 8, member=300, device=device)
    assert api.bam_probe(paths["X"], lib=lib)["paired"] == 0 and api.bam_probe(paths["X"], lib=lib, rg=WANTED)["paired"] == 1
    assert api.bam_read_groups(paths["X"], lib=lib) == ["lane1", "lane2", "other"]


def check_front_end_chunks(lib, tmp, device=0):
    # megabytes of payload, so that the chunks are chunks of payload: 6000 pairs of another group lead, and the first chunk at least selects nothing -- the front
    # end counts the chunks that hold records and keep none, so this is asserted, in every slot mode
    X, first = tagged_stream(3000, (b"lane1", b"other", b"lane2", b"x4"), prefix_pairs=6000)
    check_front_end(lib, X, first, tmp, "chunks", (b"lane1", b"lane2"), True, 250, 1000, least_chunks=3, least_empty=1, device=device)


def check_front_end_golden(lib, g, tmp, device=0, modes=(0, 1, 2)):
    """golden `qc` with two interleaved groups and OQ on most records: under selection, and with OQ alone"""
    X, first = golden_tagged(g)
    max_len = max(160, (max(len(sq) for f in (g["fq1"], g["fq2"]) for _, sq, _ in tbi.fastq_records(f)) + 15) // 16 * 16)
    batch = g["batch"]
    chunk = max(batch, g["n_pairs"] // 3 // batch * batch)
    check_front_end(lib, X, first, tmp, "qc_rg", (b"b",), False, batch, chunk, modes=modes, device=device, max_len=max_len)
    check_front_end(lib, X, first, tmp, "qc_oq", (), True, batch, chunk, modes=modes, device=device, max_len=max_len)


def test_front_end_batches_under_selection_equal_those_of_the_selected_file(emu_lib, tmp_path):
    check_front_end_small(emu_lib, str(tmp_path))


def test_front_end_stream_whose_first_chunk_selects_nothing(emu_lib, tmp_path):
    check_front_end_chunks(emu_lib, str(tmp_path))


def test_front_end_on_the_golden_under_selection_and_with_oq(golden_cases, emu_lib, tmp_path):
    check_front_end_golden(emu_lib, golden_cases["qc"], str(tmp_path))


def test_front_end_refusals_name_the_record_of_the_whole_file(emu_lib, tmp_path):
    hdr = tbi.bam_header()
    for k, (what, pay, ids, oq, bad) in enumerate(refusal_cases()):
        if bad[1] not in ("aux", "oq"):
            continue
        path = str(tmp_path / ("bad%d.bam" % k))
        open(path, "wb").write(tbi.bgzf(hdr + pay, member=120))
        fe = api.BamFrontEnd(path, batch_pairs=2, chunk_pairs=4, lib=emu_lib, rg=ids, oq=oq)
        with pytest.raises(api.FastquickError) as ei:
            tbi.drain(fe, False)
        fe.close()
        word = "auxiliary fields cannot be walked" if bad[1] == "aux" else "OQ does not fit the read"
        assert "BAM record %d:" % bad[0] in str(ei.value) and word in str(ei.value), (what, str(ei.value))


# ---- 3. the command line ----------------------------------------------------------------------------------------------------------------------------
def golden_tagged(g):
    """the golden's reads as an unaligned BAM whose pairs carry two interleaved groups, half of the records OQ -- the sequencer's qualities -- beside a QUAL that was rewritten"""
    pay, first, _ = tbi.golden_bam(g)
    recs, _, _ = tbi.split_records(pay, first)
    hdr = tbi.bam_header(text="@HD\tVN:1.6\tSO:unsorted\n@RG\tID:a\tSM:s\n@RG\tID:b\tSM:s\tLB:l\n")
    out = [hdr]
    for i, (_, r) in enumerate(recs):
        f = tbi.fields(r)
        at = 36 + f["l_name"] + 4 * f["n_cig"] + (f["l_seq"] + 1) // 2
        qual = r[at:at + f["l_seq"]]
        tags = b"NMC\x00" + Z(b"RG", b"a" if (i // 2) % 2 == 0 else b"b")
        if (i // 2) % 4 < 2 or i % 2:
            tags += Z(b"OQ", bytes(q + 33 for q in qual))
            qual = bytes(min(q, 25) for q in qual)
        body = r[4:at] + qual + tags
        out.append(struct.pack("<I", len(body)) + body)
    return b"".join(out), len(hdr)


def check_cli_same(exe, g, tmp, tag, side_a, side_b, names, timeout=None, sorted_too=True, bam_too=True):
    """two command lines, byte for byte: SAM text, the 13 QC files (.FASTQ.csv naming names[1] where the first run names names[0]), BAM payload, sorted BAM and index"""
    ins = (("_a", side_a), ("_b", side_b))
    sam = [tbi.run_cli(exe, g, os.path.join(tmp, tag + k), inp, "--sam_out", timeout=timeout) for k, inp in ins]
    assert sam[0].stdout == sam[1].stdout and any(ln and not ln.startswith(b"@") for ln in sam[0].stdout.split(b"\n")), tag
    n_qc = 0
    for name in tbi.QC_FILES:
        a, b = (open(os.path.join(tmp, tag + k + "." + name), "rb").read() for k, _ in ins)
        if name == "FASTQ.csv":
            for old in names[0]:
                a = a.replace(os.path.basename(old).encode(), os.path.basename(names[1]).encode())
        assert a == b, (tag, name)
        n_qc += 1
    assert n_qc == 13
    if bam_too:
        for k, inp in ins:
            tbi.run_cli(exe, g, os.path.join(tmp, tag + "_u" + k), inp, *(["--sorted_bam"] if sorted_too else []), timeout=timeout)
        ext = ".sorted.bam" if sorted_too else ".bam"
        assert tbi.bgzf_payload(os.path.join(tmp, tag + "_u_a" + ext)) == tbi.bgzf_payload(os.path.join(tmp, tag + "_u_b" + ext)), tag
        if sorted_too:
            assert open(os.path.join(tmp, tag + "_u_a.sorted.bam.bai"), "rb").read() == open(os.path.join(tmp, tag + "_u_b.sorted.bam.bai"), "rb").read(), tag
    return sam[1].stderr


def write_bam(tmp, name, payload):
    path = os.path.join(tmp, name)
    open(path, "wb").write(tbi.bgzf(payload))
    return path


def check_cli_rg(exe, g, tmp, timeout=None, collate=False, sorted_too=True):
    """`--bam_in X --bam_rg a [--collate]` against `--bam_in X_sel [--collate]`"""
    X, first = golden_tagged(g)
    if collate:
        X = tbc.shuffle_like_the_seeded_stream(X, first)
    s = select(X, first, (b"a",))
    assert s["unselected"] > 100 and len(s["ords"]) > 100
    px, ps = write_bam(tmp, "rg%d_X.bam" % collate, X), write_bam(tmp, "rg%d_Xsel.bam" % collate, s["X_sel"])
    extra = ["--collate"] if collate else []
    err = check_cli_same(exe, g, tmp, "rg%d" % collate, ["--bam_in", ps] + extra, ["--bam_in", px, "--bam_rg", "a"] + extra, ([ps], px), timeout=timeout, sorted_too=sorted_too)
    assert b"NOTICE - BAM input on the device: %d records (" % s["records"] in err, err.decode(errors="replace")[-2000:]
    assert b"NOTICE - BAM input, auxiliary fields walked on the device: %d records of other read groups left out, 0 records with their quality line from OQ" % s["unselected"] in err
    return px


def check_cli_oq(exe, g, tmp, timeout=None, collate=False, rg=()):
    """`--bam_in X --bam_oq [--bam_rg ..] [--collate]` against the FASTQ run on the texts of X_sel (of its collated file) under the OQ rule"""
    X, first = golden_tagged(g)
    if collate:
        X = tbc.shuffle_like_the_seeded_stream(X, first)
    s = select(X, first, rg, True)
    C = tbc.walk(s["X_sel"], first)["C"] if collate else s["X_sel"]
    paths, t = tbi.write_texts(oq_as_qual(C, first), first, tmp, "oq%d" % collate)
    px = write_bam(tmp, "oq%d_X.bam" % collate, X)
    opts = ["--bam_oq"] + [x for i in rg for x in ("--bam_rg", i.decode())] + (["--collate"] if collate else [])
    err = check_cli_same(exe, g, tmp, "oq%d" % collate, ["--fastq_1", paths[0], "--fastq_2", paths[1]], ["--bam_in", px] + opts, (paths, px), timeout=timeout, sorted_too=False)
    assert not collate or b"records without a mate" in err
    assert b"left out, %d records with their quality line from OQ" % (2 * t["units"] - count_without_oq(C, first)) in err, err.decode(errors="replace")[-1500:]


def count_without_oq(payload, first):
    return sum(1 for _, r in tbi.split_records(payload, first)[0] if not tbi.fields(r)["flag"] & 0x900 and aux_walk(r)[2] is None)


def test_command_line_selection_equals_the_run_on_the_selected_file(golden_cases, emu_cli, tmp_path):
    check_cli_rg(emu_cli, golden_cases["qc"], str(tmp_path))


def test_command_line_oq_equals_the_fastq_run_on_the_texts_with_oq(golden_cases, emu_cli, tmp_path):
    check_cli_oq(emu_cli, golden_cases["qc"], str(tmp_path))


def test_command_line_oq_and_selection_under_collation(golden_cases, emu_cli, tmp_path):
    check_cli_oq(emu_cli, golden_cases["qc"], str(tmp_path), collate=True, rg=(b"b",))


def test_command_line_without_the_options_reads_the_tagged_file_as_before(golden_cases, emu_cli, tmp_path):
    g = golden_cases["qc"]
    X, _ = golden_tagged(g)
    tbi.check_cli_equality(emu_cli, g, X, str(tmp_path), "plain", sorted_too=False)      # (the equality of 5d, its NOTICE included; the second NOTICE is absent)
    run = tbi.run_cli(emu_cli, g, str(tmp_path / "again"), ["--bam_in", str(tmp_path / "plain_X.bam")], "--sam_out")
    assert b"auxiliary fields walked" not in run.stderr


def test_command_line_refusals(golden_cases, emu_cli, tmp_path):
    g = golden_cases["qc"]
    X, _ = golden_tagged(g)
    px = write_bam(str(tmp_path), "X.bam", X)
    fq = ["--fastq_1", g["fq1"], "--fastq_2", g["fq2"]]
    for inputs, extra, words in ((fq, ["--bam_rg", "a"], [b"--bam_rg", b"--bam_in"]), (fq, ["--bam_oq"], [b"--bam_oq", b"--bam_in"]),
                                 (["--bam_in", px], ["--bam_rg", "a", "--bam_rg", "lane9"], [b"--bam_rg lane9", b"a, b"]),
                                 (["--bam_in", px], ["--bam_rg", "A"], [b"--bam_rg A", b"a, b"])):
        run = tbi.run_cli(emu_cli, g, str(tmp_path / "r"), inputs, *extra, ok=False)
        assert run.returncode != 0 and all(w in run.stderr for w in words) and not run.stdout, (extra, run.stderr[-600:])
        assert b"front end on the device" not in run.stderr      # (said before any device work)
    # a header without @RG lines
    plain = write_bam(str(tmp_path), "plain.bam", tbi.golden_bam(g)[0])
    run = tbi.run_cli(emu_cli, g, str(tmp_path / "r"), ["--bam_in", plain], "--bam_rg", "a", ok=False)
    assert run.returncode != 0 and b"no @RG line" in run.stderr
    # --RG still names the output's group
    tbi.run_cli(emu_cli, g, str(tmp_path / "rg"), ["--bam_in", px], "--bam_rg", "b", "--RG", "@RG\\tID:out\\tSM:x")
    out = tbi.bgzf_payload(str(tmp_path / "rg.bam"))
    assert b"@RG\tID:out\tSM:x" in out and b"RGZout\0" in out and b"RGZb\0" not in out


def merged_by_key(paths):
    """the records of coordinate-sorted BAM files merged in key order (reference id with -1 last, position), ties by file; the first file's header with the others' @RG lines"""
    pays = [tbi.bgzf_payload(p) for p in paths]
    firsts = [tbi.bam_first_record(p)[0] for p in pays]
    l_text = struct.unpack_from("<i", pays[0], 4)[0]
    text = pays[0][8:8 + l_text]
    for p in pays[1:]:
        lt = struct.unpack_from("<i", p, 4)[0]
        text += b"".join(ln + b"\n" for ln in p[8:8 + lt].split(b"\n") if ln.startswith(b"@RG"))
    streams = []
    for k, (p, f) in enumerate(zip(pays, firsts)):
        recs, end, flag = tbi.split_records(p, f)
        assert flag == 0 and end == len(p)
        streams.append([((struct.unpack_from("<I", r, 4)[0], struct.unpack_from("<i", r, 8)[0], k, j), r) for j, (_, r) in enumerate(recs)])
        assert streams[-1] == sorted(streams[-1], key=lambda x: x[0])
    return b"BAM\1" + struct.pack("<i", len(text)) + text + pays[0][8 + l_text:firsts[0]] + b"".join(r for _, r in heapq.merge(*streams, key=lambda x: x[0]))


def check_cli_round_trip(exe, g, tmp, timeout=None):
    """two runs with --RG a / --RG b and --sorted_bam, merged: `--bam_in M --collate --bam_rg a` equals `--bam_in Oa.sorted.bam --collate`"""
    for k in "ab":
        tbi.run_cli(exe, g, os.path.join(tmp, "rt" + k), ["--fastq_1", g["fq1"], "--fastq_2", g["fq2"]], "--sorted_bam", "--RG", "@RG\\tID:%s\\tSM:x" % k, timeout=timeout)
    Oa, Ob = (os.path.join(tmp, "rt%s.sorted.bam" % k) for k in "ab")
    M = write_bam(tmp, "M.bam", merged_by_key([Oa, Ob]))
    check_cli_same(exe, g, tmp, "rt", ["--bam_in", Oa, "--collate"], ["--bam_in", M, "--collate", "--bam_rg", "a"], ([Oa], M), timeout=timeout, bam_too=False)


def test_command_line_round_trip_of_two_merged_runs(golden_cases, emu_cli, tmp_path):
    check_cli_round_trip(emu_cli, golden_cases["qc"], str(tmp_path))


# ---- 4. the host code under AddressSanitizer / UBSan: a program of its own ------------------------------------------------------------------------
def write_check_corpus(path):
    """the entry corpus with the yardstick's results, as tests/bam_tags_check reads it: per case the payload, the IDs, the OQ flag, adjacent or collating, and
    what must come out -- the first refusal, the units, the two texts, the counts"""
    cases = []
    pay = good_payload()
    for ids, oq in ((WANTED, False), ((), True), (WANTED, True), ((b"nobody",), False)):
        cases.append((pay, ids, oq, 0))
    cases.append((pay[:len(pay) - 70], WANTED, True, 0))
    for _, p, ids, oq, _ in refusal_cases():
        cases.append((p, ids, oq, 0))
    for _, p, ids, oq in collate_payloads():
        cases.append((p, ids, oq, 1))
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for p, ids, oq, collate in cases:
            if collate:
                s = select(p, 0, ids, oq)
                w = tbc.walk(s["X_sel"], 0)
                bad = first_bad(s["tag_bad"] + ([(s["ords"][w["bad"][0]], w["bad"][1])] if w["bad"] else []))
                t = tbi.transcode(oq_as_qual(w["C"], 0) if oq else w["C"], 0) if not bad else dict(text1=b"", text2=b"")
                units, unsel = w["pairs"], s["unselected"]
            else:
                t = want_transcode(p, 0, ids, oq)
                bad, units, unsel = t["bad"], t["units"], t["unselected"]
            bad = bad or (-1, None)
            t1, t2 = t["text1"] or b"", t["text2"] or b""
            blob = b"".join(i + b"\0" for i in ids)
            fh.write(struct.pack("<iiiiq", len(ids), len(blob), int(oq), collate, len(p)) + blob + p)
            fh.write(struct.pack("<qiqqqq", bad[0], KIND_RANK.get(bad[1], 0), units, unsel, len(t1), len(t2)) + t1 + t2)
    return len(cases)


def test_host_code_under_sanitizers(tmp_path):
    subprocess.check_call(["make", "-s", "-j8", "-C", CHECK_DIR, "bam_tags_check"])      # (an object per source: the compilers run side by side)
    corpus = str(tmp_path / "corpus.bin")
    n_cases = write_check_corpus(corpus)
    X, first = tagged_stream(6000, (b"lane1", b"other", b"lane2", b"x4"), prefix_pairs=6000)
    bam = str(tmp_path / "stream.bam")
    open(bam, "wb").write(tbi.bgzf(X))
    run = subprocess.run([os.path.join(CHECK_DIR, "bam_tags_check"), corpus, bam, "500", "2000", "lane1", "lane2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    assert b"ok: %d cases, 3000 pairs" % n_cases in run.stdout, run.stdout


# ---- 5. GPU tier: every check a process of its own under a time limit -------------------------------------------------------------------------------
def gpu_step(*args, env=None):
    run = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=tbi.GPU_STEP_SEC, env=dict(os.environ, **(env or {})))
    assert run.returncode == 0, (run.stdout.decode(errors="replace")[-1500:], run.stderr.decode(errors="replace")[-3000:])
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [None, "pieces"])
def test_kernel_entry_on_the_gpu(fill):
    gpu_step("entry", env={"FASTQUICK_BAM_FILL": fill} if fill else None)


@pytest.mark.gpu
def test_collating_entry_on_the_gpu():
    gpu_step("collate", env={"FASTQUICK_BAM_HASH_BITS": "0"})


@pytest.mark.gpu
def test_front_end_on_the_gpu(tmp_path):
    gpu_step("frontend", str(tmp_path))


@pytest.mark.gpu
def test_front_end_on_the_golden_on_the_gpu(golden_cases, tmp_path):
    gpu_step("golden", golden_cases["qc"]["dir"], "qc", str(tmp_path))


@pytest.mark.gpu
def test_command_line_selection_on_the_gpu(golden_cases, tmp_path):
    check_cli_rg(tbi.CLI_GPU, golden_cases["qc"], str(tmp_path), timeout=tbi.GPU_STEP_SEC, collate=True, sorted_too=True)


@pytest.mark.gpu
def test_command_line_oq_on_the_gpu(golden_cases, tmp_path):
    check_cli_oq(tbi.CLI_GPU, golden_cases["qc"], str(tmp_path), timeout=tbi.GPU_STEP_SEC)


if __name__ == "__main__":
    lib = api.load_library()
    what = sys.argv[1]
    if what == "entry":
        check_entry_corpus(lib)
    elif what == "collate":
        check_collate_corpus(lib)
    elif what == "frontend":
        check_front_end_small(lib, sys.argv[2])
    elif what == "golden":
        g = golden_util.case_params(sys.argv[3])
        d = sys.argv[2]
        g.update(dir=d, fq1=os.path.join(d, "reads_1.fq"), fq2=os.path.join(d, "reads_2.fq"))
        check_front_end_golden(lib, g, sys.argv[4])
    else:
        raise SystemExit("unknown check " + what)
