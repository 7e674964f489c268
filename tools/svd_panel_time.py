"""svd: `FASTQuick_amd svd --RefVCF` on a synthetic panel of the shipped resource's shape, 9,962 markers x 2,504 samples.

    python tools/svd_panel_time.py [--markers 9962] [--samples 2504] [--host_eval] [--no_truth] [--workdir DIR]
    python tools/svd_panel_time.py --reader device|host_loops [--scan_records 200000 --scan_sites 10000] [--chunk_bytes N]

The panel is drawn by synth.panel_genotypes and written as a plain GT VCF (`./.` has no genotype to say -1 with: those entries read as 0/0).  Prints the
command's wall time and its own per-stage times (reader, Gram + centring, iteration with its count, projection, writers), then -- unless --no_truth --
the largest distance per component of the ABI's doubles and of the printed files from numpy's float64 SVD of the centred matrix.

--reader times the readers alone (fq_svd_read_vcf against fq_svd_read_panel, no decomposition) on the same panel written as BGZF, and prints the chunked reader's
stage seconds.  With --scan_records R it then writes the scan shape -- R records x --samples, the panel's rows repeated at new positions, as BGZF -- and a
sites file naming --scan_sites of them, and times fq_svd_read_panel(scan, sites); the serial reader has no --Sites, it is timed over the whole scan file."""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fastquick_amd import api, synth  # noqa: E402

CLI = os.path.join(ROOT, "fastquick_amd", "bin", "FASTQuick_amd")


def write_vcf(path, G):
    M, N = G.shape
    cell = np.frombuffer(b"\t0/0\t0/1\t1/1", dtype=np.uint8).reshape(3, 4)
    with open(path, "wb") as f:
        f.write(b"##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("S%04d" % j for j in range(N)).encode() + b"\n")
        for i, (chrom, pos, ref, alt) in enumerate(synth.panel_sites(M)):
            f.write(("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT" % (chrom, pos, ref, alt)).encode() + cell[G[i]].tobytes() + b"\n")


def write_bgzf_vcf(path, G, records, block=2000):
    """`records` records as BGZF, written block by block: row i is G[i % M] at site i of synth.panel_sites(records)"""
    M, N = G.shape
    cell = np.frombuffer(b"\t0/0\t0/1\t1/1", dtype=np.uint8).reshape(3, 4)
    rows = [cell[G[i]].tobytes() + b"\n" for i in range(M)]
    sites = synth.panel_sites(records)
    with open(path, "wb") as f:
        head = b"##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("S%04d" % j for j in range(N)).encode() + b"\n"
        for a in range(0, records, block):
            text = head + b"".join(("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT" % sites[i]).encode() + rows[i % M] for i in range(a, min(records, a + block)))
            head = b""
            f.write(synth.bgzf_compress(text, threads=16, level=1))
    return sites


def time_reader(paths, reader, sites=None, chunk_bytes=None):
    s = api.Svd(host_eval=True, reader=reader, chunk_bytes=chunk_bytes)
    try:
        t0 = time.perf_counter()
        n = s.read_vcf(paths) if reader == "serial" else s.read_panel(paths, sites=sites)
        wall = time.perf_counter() - t0
        st = s.read_stats()
    finally:
        s.close()
    sec = " ".join("%s %.3f" % kv for kv in st["seconds"].items())
    print("  %-10s %d x %d kept in %.3f s%s" % (reader, n[0], n[1], wall, "" if reader == "serial" else "; lines %d, at sites %d, on the host %d, chunks %d, members %d (+%d host); seconds: %s" % (
        st["lines"], st["site_lines"], st["host_lines"], st["chunks"], st["members"], st["members_host"], sec)), flush=True)


def reader_main(a, d):
    G = np.maximum(synth.panel_genotypes(a.markers, a.samples, 2504), 0).astype(np.int8)
    vcf = os.path.join(d, "panel.vcf.gz")
    write_bgzf_vcf(vcf, G, a.markers)
    print("panel %d x %d as BGZF, %.1f MB" % (a.markers, a.samples, os.path.getsize(vcf) / 1e6), flush=True)
    for rep in range(2):
        time_reader(vcf, "serial")
        time_reader(vcf, a.reader, chunk_bytes=a.chunk_bytes)
    if a.scan_records:
        scan = os.path.join(d, "scan.vcf.gz")
        t0 = time.perf_counter()
        sites = write_bgzf_vcf(scan, G, a.scan_records)
        pick = np.sort(np.random.default_rng(3).choice(a.scan_records, size=min(a.scan_sites, a.scan_records), replace=False))
        sel = os.path.join(d, "scan.SelectedSite.vcf")
        with open(sel, "w") as f:
            f.write("#CHROM\tPOS\tID\tREF\tALT\n" + "".join("%s\t%d\t.\t%s\t%s\n" % sites[i] for i in pick))
        print("scan shape %d records x %d, %d sites, BGZF %.1f MB (written in %.0f s)" % (a.scan_records, a.samples, len(pick), os.path.getsize(scan) / 1e6, time.perf_counter() - t0), flush=True)
        time_reader(scan, a.reader, sites=sel, chunk_bytes=a.chunk_bytes)
        time_reader(scan, a.reader, sites=sel, chunk_bytes=a.chunk_bytes)
        time_reader(scan, "serial")
    return 0


def column_errors(T_v, T_ud, v, ud):
    ev, eu = [], []
    for c in range(10):
        s = 1.0 if float(v[:, c] @ T_v[:, c]) >= 0 else -1.0
        ev.append(float(np.abs(s * v[:, c] - T_v[:, c]).max()))
        eu.append(float(np.abs(s * ud[:, c] - T_ud[:, c]).max()))
    return max(ev), max(eu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markers", type=int, default=9962)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--host_eval", action="store_true")
    ap.add_argument("--no_truth", action="store_true")
    ap.add_argument("--workdir")
    ap.add_argument("--reader", choices=["device", "host_loops"])
    ap.add_argument("--scan_records", type=int, default=0)
    ap.add_argument("--scan_sites", type=int, default=10000)
    ap.add_argument("--chunk_bytes", type=int)
    a = ap.parse_args()
    if a.reader:
        with tempfile.TemporaryDirectory(dir=a.workdir) as d:
            return reader_main(a, d)
    with tempfile.TemporaryDirectory(dir=a.workdir) as d:
        G = np.maximum(synth.panel_genotypes(a.markers, a.samples, 2504), 0).astype(np.int8)
        vcf = os.path.join(d, "panel.vcf")
        write_vcf(vcf, G)
        print("panel %d x %d, VCF %.1f MB" % (a.markers, a.samples, os.path.getsize(vcf) / 1e6), flush=True)
        for rep in range(2):
            t0 = time.perf_counter()
            run = subprocess.run([CLI, "svd", "--RefVCF", vcf] + (["--host_eval"] if a.host_eval else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            wall = time.perf_counter() - t0
            if run.returncode:
                print(run.stderr.decode()[-2000:])
                return 1
            note = [ln for ln in run.stderr.decode().splitlines() if "sigma_0" in ln]
            print("run %d: wall %.3f s; %s" % (rep + 1, wall, note[0] if note else "?"), flush=True)
        if a.no_truth:
            return 0
        t0 = time.perf_counter()
        X = G.astype(np.float64)
        mu = (X.sum(axis=1).astype(np.float32) / np.float32(a.samples)).astype(np.float64)
        U, S, Vt = np.linalg.svd(X - mu[:, None], full_matrices=False)
        T_v, T_ud = Vt[:10].T, U[:, :10] * S[:10]
        print("numpy float64 SVD: %.1f s; sigma %s; ratios sigma_(c+1)/sigma_c %s" % (time.perf_counter() - t0, " ".join("%.5g" % x for x in S[:11]),
                                                                                   " ".join("%.4f" % (S[c + 1] / S[c]) for c in range(10))), flush=True)
        s = api.Svd(host_eval=a.host_eval)
        s.set_genotypes(G)
        r = s.run()
        s.close()
        ev, eu = column_errors(T_v, T_ud, r["v"], r["ud"])
        print("ABI doubles:   max column error V %.3g, UD %.3g (max|UD| %.3g); %d iterations, residual %.3g, seconds %s" % (ev, eu, np.abs(T_ud).max(), r["iterations"], r["residual"], r["seconds"]))
        pv = np.array([ln.split("\t")[1:11] for ln in open(vcf + ".V")], dtype=np.float64)
        pu = np.array([ln.split("\t")[:10] for ln in open(vcf + ".UD")], dtype=np.float64)
        ev, eu = column_errors(T_v, T_ud, pv, pu)
        print("printed files: max column error V %.3g, UD %.3g (six digits of %%g)" % (ev, eu))
    return 0


if __name__ == "__main__":
    sys.exit(main())
