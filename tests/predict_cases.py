"""Helpers shared by tests/test_predict_cpu.py and tests/test_gpu_predict.py."""


def strip_labels(src, dst):
    """behaviors.tsv without the '-<label>' of every candidate token (the form
    of MIND's test split)."""
    with open(src) as f, open(dst, "w") as g:
        for line in f:
            cols = line.rstrip("\n").split("\t")
            cols[4] = " ".join(t.split("-")[0] for t in cols[4].split())
            g.write("\t".join(cols) + "\n")
