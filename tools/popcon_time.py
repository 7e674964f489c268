"""pop+con: likelihood evaluations per second of the two evaluators (fq_popcon.h) on the shape the reference was timed on: 9,962 markers at
depth 30, NumPC 4, between-ancestry model.

    python tools/popcon_time.py [--markers 9962] [--depth 30] [--num_pc 4] [--host_threads 16] [--only host|device] [--workdir DIR]

The SVD files are this script's own random numbers (the reference's resource files are not needed): allele frequencies of the shape of the
1000 Genomes panel's, a pileup drawn as a mixture of two genotype vectors.  Prints, per evaluator, the run's wall time, its evaluations and
evaluations per second, and the estimate; the two estimates are compared."""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastquick_amd import api  # noqa: E402


def make_inputs(d, n, depth, k, seed=11):
    rng = np.random.default_rng(seed)
    ud = rng.normal(0, 2.5, (n, k))
    mu = 2 * rng.beta(0.6, 0.9, n).clip(0.02, 0.98)
    pre = os.path.join(d, "svd")
    letters = "ACGT"
    bed = []
    with open(pre + ".UD", "w") as fu, open(pre + ".mu", "w") as fm, open(pre + ".bed", "w") as fb:
        for i in range(n):
            chrom, pos = str(1 + i * 22 // n), 10000 + 137 * i
            r = letters[rng.integers(4)]
            a = letters[(letters.index(r) + 1 + rng.integers(3)) % 4]
            bed.append((chrom, pos, r, a))
            fu.write("\t".join("%.6g" % x for x in ud[i]) + "\t\n")
            fm.write("%s:%d\t%.5f\n" % (chrom, pos, mu[i]))
            fb.write("%s\t%d\t%d\t%s\t%s\n" % (chrom, pos - 1, pos, r, a))
    pcs = [np.array([-0.02, 0.01, 0.004, -0.006][:k]), np.array([0.012, -0.018, -0.003, 0.005][:k])]
    g = [rng.binomial(2, np.clip((ud @ pc + mu) / 2, 0.00005, 0.99995)) for pc in pcs]
    quals = np.frombuffer(b"5:?DFIJ", dtype=np.uint8)
    with open(os.path.join(d, "mix.pileup"), "w") as f:
        for i, (chrom, pos, r, a) in enumerate(bed):
            dd = int(rng.poisson(depth))
            src = rng.random(dd) < 0.05
            alt = rng.random(dd) < np.where(src, g[0][i], g[1][i]) / 2.0
            fwd = rng.random(dd) < 0.5
            q = quals[rng.integers(len(quals), size=dd)]
            b = np.where(alt, np.where(fwd, ord(a), ord(a.lower())), np.where(fwd, ord("."), ord(","))).astype(np.uint8)
            f.write("%s\t%d\t%s\t%d\t%s\t%s\n" % (chrom, pos, r, dd, b.tobytes().decode(), q.tobytes().decode()))
    return pre, os.path.join(d, "mix.pileup")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markers", type=int, default=9962)
    ap.add_argument("--depth", type=float, default=30.0)
    ap.add_argument("--num_pc", type=int, default=4)
    ap.add_argument("--host_threads", type=int, default=16)
    ap.add_argument("--raw_evals", type=int, default=20000, help="single-point evaluations of the steady loop on the device (a twentieth of it on the host)")
    ap.add_argument("--only", choices=["host", "device"])
    ap.add_argument("--workdir")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.workdir) as d:
        svd, pileup = make_inputs(d, a.markers, a.depth, a.num_pc)
        res = {}
        for mode in ("host", "device"):
            if a.only and a.only != mode:
                continue
            t0 = time.perf_counter()
            e = api.Popcon(svd_prefix=svd, num_pc=a.num_pc, host_eval=mode == "host", host_threads=a.host_threads)
            e.set_pileup_file(pileup)
            e.llk([[0.0] * (2 * a.num_pc) + [0.5]])      # (readers, packing, upload: the first evaluation has them behind it)
            t1 = time.perf_counter()
            r = e.run()
            t2 = time.perf_counter()
            # the estimate is a short window: the same evaluator over single points in a steady loop (P = 1, what the minimiser's serial steps cost), and in batches
            n = a.raw_evals if mode == "device" else max(a.raw_evals // 20, 50)
            pts = np.zeros((n, 2 * a.num_pc + 1))
            pts[:, :2 * a.num_pc] = np.random.default_rng(5).normal(0, 0.02, (n, 2 * a.num_pc))
            pts[:, -1] = np.random.default_rng(6).uniform(0.01, 0.4, n)
            e.set_pileup_file(pileup)
            e.llk(pts[:2])
            t3 = time.perf_counter()
            one = [e.llk(p)[0] for p in pts]
            t4 = time.perf_counter()
            many = e.llk(pts)
            t5 = time.perf_counter()
            assert np.array_equal(np.array(one), many)
            print("%-6s steady: %d single-point evaluations in %.3f s (%.1f /s); the same points in batches in %.3f s (%.1f /s)" % (mode, n, t4 - t3, n / (t4 - t3), t5 - t4, n / (t5 - t4)), flush=True)
            e.close()
            res[mode] = r
            print("%-6s set-up %.3f s, estimate %.3f s: %d evaluations, %.1f evaluations/s (%d markers x depth %g, NumPC %d%s); FREEMIX %.6g llk1 %.10g"
                  % (mode, t1 - t0, t2 - t1, r["n_eval"], r["n_eval"] / (t2 - t1), a.markers, a.depth, a.num_pc, ", %d threads" % a.host_threads if mode == "host" else "",
                     min(r["alpha"], 1 - r["alpha"]), r["llk1"]), flush=True)
        if len(res) == 2:
            print("FREEMIX device - host: %.3g; evaluations %d / %d" % (res["device"]["alpha"] - res["host"]["alpha"], res["device"]["n_eval"], res["host"]["n_eval"]))


if __name__ == "__main__":
    main()
