"""Makes the inputs of tests/golden/_popcon (run by hand, see README.md): subsets of VerifyBamID2's 1000g.phase3.10k.b37 .UD/.mu/.bed resource and
pileups drawn from them, then -- with the generator's binary -- the goldens themselves.

    python make_fixtures.py RESOURCE_PREFIX [POPCON_GEN_BINARY]

Everything is seeded: a second run writes the same bytes."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
QUALS = [ord(c) for c in "5:?DFIJ"]      # Phred 20..41, the letters of a present-day instrument


def subset(prefix, idx, out, n_col=4):
    for ext in (".UD", ".mu", ".bed"):
        with open(prefix + ext) as f:
            lines = f.read().splitlines()
        with open(out + ext, "w") as f:
            for i in idx:
                f.write(("\t".join(lines[i].split()[:n_col]) + "\t" if ext == ".UD" else lines[i]) + "\n")


def load(prefix):
    ud = np.loadtxt(prefix + ".UD", ndmin=2)
    mu = np.array([float(l.split()[1]) for l in open(prefix + ".mu")])
    bed = [l.split() for l in open(prefix + ".bed")]
    return ud, mu, bed


def af_of(ud, mu, pc):
    return np.clip((ud[:, :len(pc)] @ np.asarray(pc) + mu) / 2.0, 0.00005, 0.99995)


def draw_pileup(path, ud, mu, bed, pc_a, pc_b, alpha, mean_depth, seed, drop=()):
    """reads of a mixture: a fraction alpha from a genotype vector drawn at pc_a's allele frequencies, the rest from one drawn at pc_b's"""
    rng = np.random.default_rng(seed)
    ga = rng.binomial(2, af_of(ud, mu, pc_a))
    gb = rng.binomial(2, af_of(ud, mu, pc_b))
    with open(path, "w") as f:
        for i, (chrom, _, pos, ref, alt) in enumerate(bed):
            if i in drop:
                continue
            d = int(rng.poisson(mean_depth))
            bases, quals = [], []
            for _ in range(d):
                g = ga[i] if rng.random() < alpha else gb[i]
                q = QUALS[rng.integers(len(QUALS))]
                is_alt = rng.random() < g / 2.0
                fwd = rng.random() < 0.5
                if rng.random() < 10 ** (-(q - 33) / 10.0):      # a sequencing error: one of the three other letters
                    others = [c for c in "ACGT" if c != (alt if is_alt else ref)]
                    b = others[rng.integers(3)]
                    b = ("." if fwd else ",") if b == ref else (b if fwd else b.lower())
                elif is_alt:
                    b = alt if fwd else alt.lower()
                else:
                    b = "." if fwd else ","
                bases.append(b)
                quals.append(chr(q))
            f.write("%s\t%s\t%s\t%d\t%s\t%s\n" % (chrom, pos, ref, d, "".join(bases), "".join(quals)))


def edge_pileup(path, bed):
    """130 markers, hand made: marker i of the .bed on line order below; see README.md for what each is there for"""
    rng = np.random.default_rng(99)
    qs = "!+5?IJ~"

    def line(i, d, bases=None, quals=None, depth_col=None):
        chrom, _, pos, ref, alt = bed[i]
        if bases is None:
            bases = "".join(rng.choice([".", ",", alt, alt.lower(), "N", "n", "A", "c", "*"], p=[.3, .3, .12, .12, .04, .02, .04, .04, .02]) for _ in range(d))
        if quals is None:
            quals = "".join(qs[rng.integers(len(qs))] for _ in range(d))
        return "%s\t%s\t%s\t%d\t%s\t%s\n" % (chrom, pos, ref, d if depth_col is None else depth_col, bases, quals)

    out = []
    for i in range(130):
        chrom, _, pos, ref, alt = bed[i]
        if i == 5:
            continue                                   # an absent marker
        if i == 6:
            out.append("%s\t%s\t%s\t0\t\t\n" % (chrom, pos, ref))     # a zero-depth line: no bases, no qualities
        elif i == 7:
            out.append(line(i, 1))
        elif i == 10:
            out.append(line(i, 4))                     # a duplicated site: its second line follows further down
        elif i == 11:
            out.append(line(i, 6, depth_col=9))        # the depth column says more than the strings hold
        elif i == 12:
            out.append(line(i, 5, quals="!!!!!"))
        elif i == 13:
            out.append(line(i, 5, quals="~~~~~"))
        elif i == 14:
            out.append(line(i, 6, bases=alt.lower() * 3 + "N" + "n" + "."))
        elif i in (63, 64, 65):
            out.append(line(i, i))
        elif i == 70:
            out.append(line(i, 300))
        elif i == 71:
            out.append(line(i, 40, bases="N" * 40, quals="~" * 40))   # every genotype pair's product underflows: markerLK == 0
        else:
            out.append(line(i, int(rng.integers(2, 30))))
        if i == 20:
            out.append("%s\t%d\t%s\t3\t.,.\tIII\n" % (chrom, int(pos) + 1, ref))   # a site the .bed does not hold
        if i == 40:
            out.append(line(10, 3))                    # the duplicate of marker 10
    out.append("notachrom\t12345\tA\t2\t..\tII\n")
    with open(path, "w") as f:
        f.write("".join(out))


CASES = [
    # name, svd, pileup, num_pc, generator options
    ("mix_a", "svd1200", "mix_a.pileup", 2, []),
    ("mix_b", "svd1200", "mix_b.pileup", 2, []),
    ("numpc4", "svd1200", "mix_a.pileup", 4, []),
    ("within", "svd1200", "mix_b.pileup", 2, ["within"]),
    ("numpc1", "svd1200", "mix_b.pileup", 1, ["within"]),
    ("fixalpha", "svd1200", "mix_a.pileup", 2, ["fixalpha=0.05"]),
    ("fixpc", "svd1200", "mix_a.pileup", 2, ["fixpc=-0.02:0.01"]),
    ("knownaf", "svd1200", "mix_b.pileup", 2, ["knownaf=svd1200.af"]),
    ("swap", "svd1200", "mix_a.pileup", 2, ["fixalpha=0.7"]),
    ("swapfree", "svd1200", "mix_a.pileup", 2, ["fixpc=-0.028:0.012"]),      # the intended sample fixed at the contaminant's PCs: the estimated alpha lands at 0.92
    ("edge", "svd130", "edge.pileup", 2, ["nosanity"]),
]


def main():
    prefix = sys.argv[1]
    os.chdir(HERE)
    subset(prefix, [8 * i for i in range(1200)], "svd1200")
    ud, mu, bed = load("svd1200")
    subset("svd1200", list(range(130)), "svd130")
    pc_x, pc_y = [-0.028, 0.012], [0.015, -0.02]
    draw_pileup("mix_a.pileup", ud, mu, bed, pc_x, pc_y, 0.08, 8.0, 1, drop=(17, 400))
    draw_pileup("mix_b.pileup", ud, mu, bed, pc_y, pc_y, 0.2, 6.0, 2)
    with open("svd1200.af", "w") as f:
        for row, af in zip(bed, af_of(ud, mu, pc_y)):
            f.write("\t".join(row) + "\t%.6f\n" % af)
    edge_pileup("edge.pileup", bed)
    with open("cases.txt", "w") as f:
        for name, svd, pile, npc, opts in CASES:
            f.write("%s %s %s %d %s\n" % (name, svd, pile, npc, " ".join(opts)))
    if len(sys.argv) > 2:
        for name, svd, pile, npc, opts in CASES:
            print("==", name, flush=True)
            subprocess.run([sys.argv[2], svd, pile, name, str(npc)] + opts, check=True, stdout=subprocess.DEVNULL)
        pack()


def pack():
    """the inputs and the reference's output files into fixtures.tar.gz (tests/test_popcon.py unpacks it), names sorted, no times or owners; cases.txt and the
    recorded numbers (*.golden) stay plain files"""
    import gzip
    import tarfile
    os.chdir(HERE)
    names = sorted(f for f in os.listdir(".") if os.path.isfile(f) and f not in ("README.md", "make_fixtures.py", "fixtures.tar.gz", "cases.txt") and not f.endswith(".golden"))
    with open("fixtures.tar.gz", "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as gz, tarfile.open(fileobj=gz, mode="w") as tar:
        for f in names:
            info = tar.gettarinfo(f)
            info.mtime, info.uid, info.gid, info.uname, info.gname = 0, 0, 0, "", ""
            with open(f, "rb") as fh:
                tar.addfile(info, fh)
    for f in names:
        os.remove(f)


if __name__ == "__main__":
    main()
