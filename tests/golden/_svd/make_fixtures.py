"""Makes tests/golden/_svd (run by hand, see README.md): panel VCFs drawn by fastquick_amd.synth and -- with the generator's binary -- the four files
VerifyBamID2's SVDcalculator::ProcessRefVCF writes for each.

    python make_fixtures.py SVD_GEN_BINARY

Everything is seeded: a second run writes the same bytes."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

from fastquick_amd import synth  # noqa: E402

# name, markers, samples, FORMAT, seed
PANELS = [("p333x45", 333, 45, "GT", 4501), ("p640x96", 640, 96, "PL", 9601), ("p97x33", 97, 33, "GL", 3301), ("p40x16", 40, 16, "GT", 1601)]


def edge_vcf(path):
    """12 samples; 24 plain GT markers drawn as the panels are, and among them the lines the reader's rules are there for"""
    G = synth.panel_genotypes(24, 12, 1201)
    sites = synth.panel_sites(24 * 11)[::11]      # two markers a chromosome or so, chromosomes 1 .. 22
    gt = ("0/0", "0/1", "1/1")
    hdr = "##fileformat=VCFv4.1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("E%02d" % j for j in range(12)) + "\n"
    out = [hdr]

    def rec(chrom, pos, ref, alt, fmt, cells):
        out.append("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\t%s\t%s\n" % (chrom, pos, ref, alt, fmt, "\t".join(cells)))

    for i, (chrom, pos, ref, alt) in enumerate(sites):
        cells = [gt[max(int(g), 0)] for g in G[i]]
        if i == 2:      # an indel and a deletion: skipped
            rec(chrom, pos - 40, "AT", "A", "GT", cells)
            rec(chrom, pos - 30, "G", "GAA", "GT", cells)
        if i == 3:      # a multi-allelic site: the first ALT allele counts, allele 2 of a GT adds 2
            rec(chrom, pos, ref, alt + "," + ref.lower(), "GT", ["0/2" if j == 4 else c for j, c in enumerate(cells)])
            continue
        if i == 5:      # missing and phased genotypes: `.` reads as 0
            rec(chrom, pos, ref, alt, "GT", ["./.", ".|1", "1|.", "1|1", "0|1", "1|0", "0|0", "./1", "1|1", "0/0", "0|1", "1/0"])
            continue
        if i == 7:      # PL: one sample all 255 (genotype -1), one above the cap, a tie (the first strict minimum wins), GT ahead of PL in FORMAT
            pl = ["0,30,50", "50,0,50", "50,30,0", "255,255,255", "300,400,254", "10,10,10", "0,0,0", "255,255,0", "255,0,255", "20,3,3", "1,0,0", "60,70,80"]
            rec(chrom, pos, ref, alt, "GT:DP:PL", ["%s:7:%s" % (c, p) for c, p in zip(cells, pl)])
            continue
        if i == 9:      # GL: -10 x value truncates towards zero (-2.99 -> 29, not 30), -0.0 is 0
            gl = ["-0.0,-2.99,-5", "-2.99,-2.90,-3", "-5,-3.04,-0.09", "-25.5,-25.5,-25.5", "-25.49,-30,-30", "-0.19,-0.11,-0.1", "0,0,0", "-1,-0.05,-0.04",
                  "-3,-0.0,-3", "-4.5,-4.49,-4.41", "-26,-27,-25.4", "-0.1,-0.2,-0.3"]
            rec(chrom, pos, ref, alt, "GL", gl)
            continue
        if i == 12:     # chromosomes outside 1 .. 22: skipped (after the duplicate test, which they do not disturb)
            rec("X", 5000, "A", "C", "GT", cells)
            rec("chrM", 73, "A", "G", "GT", cells)
            rec("chrX", 5001, "A", "C", "GT", cells)
        if i == 15:     # chr-prefixed autosomes are kept
            chrom = "chr" + chrom
        rec(chrom, pos, ref, alt, "GT", cells)
        if i == 18:     # a site repeated behind another one, with other alleles: both rows stay, the .bed shows the later alleles on both
            c0, p0, r0, a0 = sites[17]
            rec(c0, p0, a0, r0, "GT", [gt[2 - max(int(g), 0)] for g in G[17]])
    with open(path, "w") as f:
        f.write("".join(out))


def main():
    gen = os.path.abspath(sys.argv[1])
    os.chdir(HERE)
    jobs = []
    for name, M, N, fmt, seed in PANELS:
        vcf = name + ".vcf.gz"
        synth.panel_vcf(vcf, synth.panel_genotypes(M, N, seed), fmt)
        jobs.append((vcf, name))
    edge_vcf("edge.vcf")
    jobs.append(("edge.vcf", "edge"))
    for vcf, name in jobs:
        print("==", name, flush=True)
        plain = vcf
        if vcf.endswith(".gz"):      # (the generator is handed the text: see README.md)
            import gzip
            plain = name + ".tmp.vcf"
            with gzip.open(vcf, "rb") as src, open(plain, "wb") as dst:
                dst.write(src.read())
        subprocess.run([gen, plain], check=True, stdout=subprocess.DEVNULL)
        for ext in (".UD", ".mu", ".V", ".bed"):
            os.replace(plain + ext, name + ext)
        if plain != vcf:
            os.remove(plain)


if __name__ == "__main__":
    main()
