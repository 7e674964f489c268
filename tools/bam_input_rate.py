#!/usr/bin/env python3
"""BAM input: pairs/s of fq_frontend_open_bam against fq_frontend_open on the same reads -- the reads of tools/frontend_ragged_check.py
(trimmed to 60..150 bases, Illumina-style names of varying length, with a comment in the FASTQ files; qualities over 40 values), written as an
unaligned BAM and as two BGZF FASTQ files --, the BAM kernels' times and chain_repairs (profiles/bam_input.txt).
    python tools/bam_input_rate.py [--pairs N] [--uniform] [--only bam|fastq] [--workdir DIR] [--root CHECKOUT]
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
ap.add_argument("--only", choices=["bam", "fastq"])
ap.add_argument("--workdir")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=3)
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

    def run(make):
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
        assert k == 0 and got == n, (k, got)
        return dt, st

    print("library of %s ; FASTQUICK_BAM_FILL=%s" % (os.path.abspath(a.root), os.environ.get("FASTQUICK_BAM_FILL", "(a wavefront per record)")), flush=True)
    for rep in range(a.reps):
        if a.only != "fastq":
            dt, st = run(lambda: api.BamFrontEnd(X, batch_pairs=262144, chunk_pairs=4 * 262144, slot_mode=0, max_read_len=160))
            print("BAM   rep %d: %.3f s, %.2f M pairs/s ; inflate %.1f ms, starts %.1f, pairs %.1f, fill %.1f, tokenise %.1f ; chunks %d, repairs %d, records %d, wait_reader %.0f ms" % (
                rep, dt, n / dt / 1e6, st["ms_inflate"], st["ms_bam_starts"], st["ms_bam_pairs"], st["ms_bam_fill"], st["ms_tokenise"], st["chunks"], st["chain_repairs"], st["bam_records"],
                st["ms_wait_reader"]), flush=True)
        if a.only != "bam":
            dt, st = run(lambda: api.DeviceFrontEnd(fq[0], fq[1], batch_pairs=262144, chunk_pairs=4 * 262144, slot_mode=0, max_read_len=160))
            print("FASTQ rep %d: %.3f s, %.2f M pairs/s ; inflate %.1f ms, tokenise %.1f ; chunks %d, wait_reader %.0f ms" % (rep, dt, n / dt / 1e6, st["ms_inflate"], st["ms_tokenise"], st["chunks"],
                                                                                                                       st["ms_wait_reader"]), flush=True)
finally:
    if not a.workdir:
        shutil.rmtree(work, ignore_errors=True)
