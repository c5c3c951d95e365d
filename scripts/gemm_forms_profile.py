"""Writes profiles/gemm_forms_mi355x.json from one GPU run of the GEMM-family tests.

    python -m pytest tests/test_gpu_gemm_forms.py -q -s > LOG
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o gemm_forms -- python -m pytest tests/test_gpu_gemm_forms.py -q
    python scripts/gemm_forms_profile.py LOG DIR/gemm_forms_kernel_stats.csv [--out profiles/gemm_forms_mi355x.json]

From LOG: per case the largest `|got - ref| / bound` that its rounded variants printed (`[gemm-forms] case | variant | ratio`; the
members of a batched case are folded into one entry).  From the kernel statistics: the launches per GEMM kernel instantiation, compared
with the counts the case table of tests/gemm_forms.py predicts (every sg_gemm case runs 3 variants, 2 behind tanh / sigmoid, plus the
NaN / Inf runs; a gemm_nt case launches its finalize unless the plan is direct)."""
import argparse
import collections
import csv
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), os.path.join(HERE, "..", "tests")]
import gemm_forms as G  # noqa: E402

MAT = {"k": "sg::MatRowMajor", "r": "sg::MatColMajor"}
KMAJOR = {"k": "true", "r": "false"}


def expected_launches():
    exp = collections.Counter()

    def gemm(c, n):
        kind, tm, tn, S, fin = c.plan
        if kind == G.SKELETON:
            exp["tile_gemm_kernel<%d, %d, %s, %s, %s>" % (tm, tn, MAT[c.la], MAT[c.lb], "sg::GemmEpi" if S == 1 else "sg::EpiWorkspace")] += n
        elif kind == G.PERSISTENT:
            exp["gemm128p_kernel<%s, %s>" % (KMAJOR[c.la], KMAJOR[c.lb])] += n
        else:
            exp["gemm128_kernel<%s, %s, %s>" % (KMAJOR[c.la], KMAJOR[c.lb], "sg::Gemm128Direct" if S == 1 else "sg::Gemm128Partial")] += n
        if fin == G.FIN_FLAT:
            exp["splitk_finalize_kernel<sg::GemmEpi>"] += n
        if fin == G.FIN_DEEP:
            exp["splitk_finalize_deep_kernel<sg::GemmEpi>"] += n

    for c in G.GEMM_CASES:
        gemm(c, 3 if c.act in (G.ACT_NONE, G.ACT_LEAKY, G.ACT_RELU) else 2)
    for i in G.NONFINITE_IDS:
        gemm(G.GEMM_BY_ID[i], 1)
    for c in G.NT_CASES:
        n = 3 + (c.id == G.NT_NONFINITE_ID)
        exp["gemm_nt_bigk_kernel<%s>" % ("true" if c.entry == "lnrelu" else "false")] += n
        if not c.plan[0]:
            exp["gemm_nt_finalize_kernel"] += n
    return exp


def traced_launches(stats_csv):
    got = collections.Counter()
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            m = re.search(r"sg::((?:tile_gemm|gemm128p?|gemm_nt_bigk|gemm_nt_finalize|splitk_finalize(?:_deep)?)_kernel(?:<.*?>)?)\(", row["Name"])
            if m:
                got[m.group(1)] += int(row["Calls"])
    return got


def ratios(log):
    out = {}
    with open(log) as f:
        for line in f:
            m = re.search(r"\[gemm-forms\] (\S+) \| (randn|scaled|nonfinite) \| (\S+)", line)
            if m:
                key = re.sub(r"\[\d+\]$", "", m.group(1))
                out[key] = max(out.get(key, 0.0), float(m.group(3)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log")
    ap.add_argument("kernel_stats_csv")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "gemm_forms_mi355x.json"))
    args = ap.parse_args()
    exp, got, r = expected_launches(), traced_launches(args.kernel_stats_csv), ratios(args.log)
    for k in sorted(set(exp) | set(got)):
        if exp[k] != got[k]:
            print("launch count differs: %s: the table predicts %d, traced %d" % (k, exp[k], got[k]))
    doc = {"what": "tests/test_gpu_gemm_forms.py on one MI355X: per case the largest |got - ref| / bound over its rounded variants (the bound "
                   "is the derived one of tests/gemm_forms.py, not tuned to these numbers; exact variants were bit-equal), and the launches "
                   "per kernel instantiation of one traced run (rocprofv3 --kernel-trace --stats) against the case table's prediction",
           "launch_counts_match_table": exp == got, "kernel_launches": dict(sorted(got.items())), "max_ratio": max(r.values()),
           "ratio_of_bound": dict(sorted(r.items()))}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("%d cases, largest ratio %.3g, %d kernel instantiations, launch counts match the table: %s" % (
        len(r), max(r.values()), len(got), exp == got))


if __name__ == "__main__":
    main()
