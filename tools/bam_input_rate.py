#!/usr/bin/env python3
"""BAM input: pairs/s of fq_frontend_open_bam against fq_frontend_open on the same reads -- the reads of tools/frontend_ragged_check.py
(trimmed to 60..150 bases, Illumina-style names of varying length, with a comment in the FASTQ files; qualities over 40 values), written as an
unaligned BAM and as two BGZF FASTQ files --, the BAM kernels' times and chain_repairs (profiles/bam_input.txt).
    python tools/bam_input_rate.py [--pairs N] [--uniform] [--only bam|fastq|collate] [--collate] [--far F] [--workdir DIR] [--root CHECKOUT]
                                   [--tagged] [--bam_rg ID]... [--bam_oq]
--tagged: the BAM legs read XT.bam -- the same records with NM, RG:Z (four groups g0..g3 interleaved pair by pair), OQ:Z (the qualities as they were; QUAL capped at 25, as a
recalibration would leave it) and a B:S array, about 190 auxiliary bytes a record -- in place of X.bam; --bam_rg / --bam_oq (DESIGN.md 5d'', profiles/bam_tags.txt): the
options of fq_frontend_open_bam_select on it, the tag kernel's time and the counts in the line;
--collate: a third leg (DESIGN.md 5d', profiles/bam_collate.txt) -- the same records in a coordinate-like order (the permutation of tests/test_bam_collate.py's seeded
stream: second mates a geometric distance behind their first, a fraction --far of them anywhere, 3 % supplementary copies, 1 % of the pairs without a mate) through
fq_frontend_open_bam_collate, and through fq_bam_collate_device for the collation kernels' time by kernel;
--root: the checkout whose fastquick_amd package (and built library) is measured -- the parent commit's build gives the FASTQ yardstick with `--only fastq`;
--workdir: where the input files are written and looked for (by default a temporary directory that is removed); FASTQUICK_BAM_FILL=pieces: the fill's other form."""
import argparse
import os
import shutil
import struct
import sys
import tempfile
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1 << 20)
ap.add_argument("--uniform", action="store_true", help="every read 150 bases (names still vary)")
ap.add_argument("--only", choices=["bam", "fastq", "collate"])
ap.add_argument("--collate", action="store_true", help="the collating leg on the permuted file")
ap.add_argument("--far", type=float, default=0.02, help="the fraction of second mates placed anywhere in the file")
ap.add_argument("--workdir")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--tagged", action="store_true", help="the BAM legs read the file whose records carry RG (four groups interleaved) and OQ")
ap.add_argument("--bam_rg", action="append", default=[], help="select this read group of the tagged file (g0..g3; repeatable)")
ap.add_argument("--bam_oq", action="store_true", help="quality lines from OQ")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
from fastquick_amd import api, synth  # noqa: E402

api.load_library().fq_runtime_configure(20, 1)
work = a.workdir or tempfile.mkdtemp(prefix="fq_bam_rate_")
os.makedirs(work, exist_ok=True)
n = a.pairs
key = "%d_%s" % (n, "u" if a.uniform else "r")
X = os.path.join(work, "X_%s.bam" % key)
fq = [os.path.join(work, "T%d_%s.fq.gz" % (e + 1, key)) for e in range(2)]
S = os.path.join(work, "S_%s_%g.bam" % (key, a.far))
collate = a.collate or a.only == "collate"
tagged = a.tagged or a.bam_rg or a.bam_oq
XT = os.path.join(work, "XT_%s.bam" % key)
GROUPS = 4


def bgzf_payload(path):
    import zlib
    blob, at, parts = open(path, "rb").read(), 0, []
    while at < len(blob):
        bsize = struct.unpack_from("<H", blob, at + 16)[0] + 1
        parts.append(zlib.decompress(blob[at + 18:at + bsize - 8], -15))
        at += bsize
    return b"".join(parts)


def write_permuted(src, dst, far_frac, seed=20261019, mean_dist=30.0):
    """src's records (mates adjacent) in a coordinate-like order; returns the pairs that keep both mates"""
    pay = bgzf_payload(src)
    first = 12 + struct.unpack_from("<i", pay, 4)[0]
    for _ in range(struct.unpack_from("<i", pay, first - 4)[0]):
        first += 8 + struct.unpack_from("<i", pay, first)[0]
    starts, p = [], first
    while p < len(pay):
        starts.append(p)
        p += 4 + struct.unpack_from("<I", pay, p)[0]
    starts.append(p)
    m = (len(starts) - 1) // 2
    rng = np.random.default_rng(seed)
    where = np.empty(2 * m)
    where[0::2] = np.arange(m) * 2.0
    where[1::2] = where[0::2] + 2.0 * rng.geometric(1.0 / mean_dist, m) - 0.5
    far = rng.random(m) < far_frac
    where[1::2][far] = rng.random(int(far.sum())) * 2.0 * m
    lost = rng.random(m) < 0.01
    sup = rng.random(2 * m) < 0.03
    out = [pay[:first]]
    for i in np.argsort(where, kind="stable"):
        if lost[i // 2] and i % 2 == (i // 2) % 2:
            continue
        r = pay[starts[i]:starts[i + 1]]
        out.append(r)
        if sup[i]:
            out.append(r[:18] + struct.pack("<H", struct.unpack_from("<H", r, 18)[0] | 0x800) + r[20:])
    with open(dst, "wb") as fh:
        fh.write(synth.bgzf_compress(b"".join(out), threads=16, level=6))
    return m - int(lost.sum())
try:
    if not all(os.path.exists(p) for p in [X] + fq):
        t0 = time.time()
        rng = np.random.default_rng(31)
        lens = [np.where(rng.random(n) < (0.0 if a.uniform else 0.3), rng.integers(60, 151, n), 150) for _ in range(2)]
        xs, ys = rng.integers(1000, 40000, n), rng.integers(1000, 200000, n)
        names = [b"A00123:45:HXXXXXXXX:1:%d:%d:%d" % (1101 + i % 1000, xs[i], ys[i]) for i in range(n)]
        recs = [[None] * n, [None] * n]
        for e in range(2):
            c = rng.integers(0, 4, (n, 150), dtype=np.uint8)
            seq = np.frombuffer(b"ACGT", dtype=np.uint8)[c].tobytes()
            qual = rng.integers(35, 75, (n, 150), dtype=np.uint8)
            code = np.array([1, 2, 4, 8], dtype=np.uint8)[c]
            packed = (code[:, 0::2] << 4 | code[:, 1::2]).astype(np.uint8).tobytes()
            q33, qtxt = (qual - 33).astype(np.uint8).tobytes(), qual.tobytes()
            text = []
            for i in range(n):
                L = int(lens[e][i])
                nm = names[i]
                text.append(b"@%s %d:N:0:ACGTACGT\n%s\n+\n%s\n" % (nm, e + 1, seq[150 * i:150 * i + L], qtxt[150 * i:150 * i + L]))
                pk = packed[75 * i:75 * i + (L + 1) // 2]
                if L & 1:
                    pk = pk[:-1] + bytes([pk[-1] & 0xf0])
                body = struct.pack("<iiBBHHHiiii", -1, -1, len(nm) + 1, 0, 4680, 0, 77 if e == 0 else 141, L, -1, -1, 0) + nm + b"\0" + pk + q33[150 * i:150 * i + L]
                recs[e][i] = struct.pack("<I", len(body)) + body
            with open(fq[e], "wb") as fo:
                fo.write(synth.bgzf_compress(b"".join(text), threads=16, level=6))
        hdr = b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 2) + b"1\0" + struct.pack("<i", 1000)
        with open(X, "wb") as fh:
            fh.write(synth.bgzf_compress(hdr + b"".join(r for pair in zip(recs[0], recs[1]) for r in pair), threads=16, level=6))
        print("files written in %.0f s: %d pairs, X.bam %.1f MB, T1 %.1f MB, T2 %.1f MB" % (time.time() - t0, n, os.path.getsize(X) / 1e6, os.path.getsize(fq[0]) / 1e6, os.path.getsize(fq[1]) / 1e6),
              flush=True)

    if tagged and not os.path.exists(XT):
        t0 = time.time()
        pay = bgzf_payload(X)
        text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@RG\tID:g%d\tSM:s\n" % k for k in range(GROUPS))
        out, p, i = [b"BAM\1" + struct.pack("<i", len(text)) + text + pay[8:22]], 22, 0      # (X's header: no text, one reference "1": 22 bytes)
        extra = b"ZBBS" + struct.pack("<I", 4) + struct.pack("<4H", 1, 2, 3, 4)
        while p < len(pay):
            bs = struct.unpack_from("<I", pay, p)[0]
            r = pay[p:p + 4 + bs]
            L = struct.unpack_from("<I", r, 20)[0]
            q = np.frombuffer(r, dtype=np.uint8, count=L, offset=4 + bs - L)
            body = r[4:4 + bs - L] + np.minimum(q, 25).tobytes() + b"NMC\0" + b"RGZg%d\0" % (i // 2 % GROUPS) + b"OQZ" + (q + 33).tobytes() + b"\0" + extra
            out.append(struct.pack("<I", len(body)) + body)
            p += 4 + bs; i += 1
        with open(XT, "wb") as fh:
            fh.write(synth.bgzf_compress(b"".join(out), threads=16, level=6))
        print("tagged file written in %.0f s: XT.bam %.1f MB" % (time.time() - t0, os.path.getsize(XT) / 1e6), flush=True)
    if tagged:
        X = XT
    n_sel = sum(1 for i in range(n) if "g%d" % (i % GROUPS) in a.bam_rg) if a.bam_rg else n
    opts = dict(rg=a.bam_rg, oq=a.bam_oq) if a.bam_rg or a.bam_oq else {}      # (a checkout from before the options takes none)

    n_S = None
    if collate:
        t0 = time.time()
        n_S = write_permuted(X, S, a.far)
        print("permuted file written in %.0f s: far %g, %d pairs with both mates, S.bam %.1f MB" % (time.time() - t0, a.far, n_S, os.path.getsize(S) / 1e6), flush=True)

    def run(make, want=None):
        fe = make()
        t0 = time.perf_counter()
        got = 0
        while True:
            k, b = fe.next()
            if k <= 0:
                break
            got += k
            fe.release(b)
        dt = time.perf_counter() - t0
        st = fe.stats()
        fe.close()
        assert k == 0 and got == (want or n), (k, got)
        return dt, st

    print("library of %s ; FASTQUICK_BAM_FILL=%s" % (os.path.abspath(a.root), os.environ.get("FASTQUICK_BAM_FILL", "(a wavefront per record)")), flush=True)
    for rep in range(a.reps):
        if a.only not in ("fastq", "collate"):
            dt, st = run(lambda: api.BamFrontEnd(X, batch_pairs=262144, chunk_pairs=4 * 262144, slot_mode=0, max_read_len=160, **opts), n_sel)
            print("BAM   rep %d: %.3f s, %.2f M pairs/s ; inflate %.1f ms, starts %.1f, pairs %.1f, fill %.1f, tokenise %.1f ; chunks %d, repairs %d, records %d, wait_reader %.0f ms" % (
                rep, dt, n_sel / dt / 1e6, st["ms_inflate"], st["ms_bam_starts"], st["ms_bam_pairs"], st["ms_bam_fill"], st["ms_tokenise"], st["chunks"], st["chain_repairs"], st["bam_records"],
                st["ms_wait_reader"]) + (" ; --bam_rg %s%s: tags %.1f ms (%.2f ms per million records), %d records unselected, %d with OQ, %.2f M records/s walked" % (
                    ",".join(a.bam_rg) or "-", " --bam_oq" if a.bam_oq else "", st["ms_bam_tags"], st["ms_bam_tags"] / (st["bam_records"] / 1e6), st["bam_unselected"], st["bam_oq_records"],
                    st["bam_records"] / dt / 1e6) if opts else ""), flush=True)
        if collate:
            dt, st = run(lambda: api.BamFrontEnd(S, batch_pairs=262144, chunk_pairs=4 * 262144, slot_mode=0, max_read_len=160, collate_mem=4 << 30), n_S)
            print("COLL  rep %d: %.3f s, %.2f M pairs/s ; inflate %.1f ms, starts %.1f, keep %.1f, collate %.1f, fill %.1f, tokenise %.1f ; chunks %d, repairs %d, records %d, orphans %d, held peak %d records %.1f MB, "
                  "wait_reader %.0f ms" % (rep, dt, n_S / dt / 1e6, st["ms_inflate"], st["ms_bam_starts"], st["ms_bam_pairs"], st["ms_bam_collate"], st["ms_bam_fill"], st["ms_tokenise"], st["chunks"],
                                           st["chain_repairs"], st["bam_records"], st["bam_orphans"], st["bam_held_peak_records"], st["bam_held_peak_bytes"] / 1e6, st["ms_wait_reader"]), flush=True)
        if a.only not in ("bam", "collate"):
            dt, st = run(lambda: api.DeviceFrontEnd(fq[0], fq[1], batch_pairs=262144, chunk_pairs=4 * 262144, slot_mode=0, max_read_len=160))
            print("FASTQ rep %d: %.3f s, %.2f M pairs/s ; inflate %.1f ms, tokenise %.1f ; chunks %d, wait_reader %.0f ms" % (rep, dt, n / dt / 1e6, st["ms_inflate"], st["ms_tokenise"], st["chunks"],
                                                                                                                       st["ms_wait_reader"]), flush=True)
    if collate:      # the collation kernels by kernel: the same chunk loop on the payload in host memory, 1024 members (64 MB) a chunk
        pay = bgzf_payload(S)
        first = 12 + struct.unpack_from("<i", pay, 4)[0]
        for _ in range(struct.unpack_from("<i", pay, first - 4)[0]):
            first += 8 + struct.unpack_from("<i", pay, first)[0]
        for rep in range(a.reps):
            r = api.bam_collate_device(pay, range(0, len(pay), 65280), 1, first, members_per_chunk=1024)
            print("KERN  rep %d: collate %.2f ms = keys %.2f + sort %.2f + match %.2f + units %.2f + held gather %.2f ; chunks %d, pairs %d, orphans %d, held peak %d records %.1f MB" % (
                rep, r["ms_collate"], r["ms_keys"], r["ms_sort"], r["ms_match"], r["ms_units"], r["ms_hold"], r["chunks"], r["pairs"], r["orphans"], r["held_peak_records"], r["held_peak_bytes"] / 1e6), flush=True)
finally:
    if not a.workdir:
        shutil.rmtree(work, ignore_errors=True)
