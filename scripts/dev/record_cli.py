"""Records what the six analysis tools print, exit with and write on the CPU, to compare two trees.

    python scripts/dev/record_cli.py LISTING.json          # run every case, write the listing
    python scripts/dev/record_cli.py --diff A.json B.json  # print the cases that differ (nothing when the trees agree)

Every case runs `python -m cryo_ralib_amd.TOOL ... --backend numpy` (sdr has no CPU path: its case records the exit) in a fresh
working directory with the same small seeded inputs, so stdout, stderr, the exit status and every array of the output .npz (dtype,
shape and the SHA-256 of its bytes) are functions of the tree alone.  The cases walk the branches the tools share: .npy and .npz
input with a good and a missing --key, --truth from an int .npy and from a params.txt (good, wrong length, an idx column that is no
permutation), --averages without --stack, a NaN, a 1-D input, and for DBSCAN / HDBSCAN a run where everything is noise and one with
some noise.  Line numbers in warnings are masked; nothing else is.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_inputs(d):
    rs = np.random.RandomState(7)
    n, dim = 240, 4
    centres = np.array([[0, 0, 0, 0], [6, 0, 1, 0], [0, 7, 0, 2]], np.float64)
    truth = np.repeat(np.arange(3), n // 3)
    X = (centres[truth] + rs.standard_normal((n, dim)) * 0.6).astype(np.float32)
    X[::40] += rs.standard_normal((n // 40, dim)).astype(np.float32) * 9.0          # a few far points: noise for the density tools
    perm = rs.permutation(n)
    X, truth = X[perm], truth[perm]
    np.save(os.path.join(d, "X.npy"), X)
    np.savez(os.path.join(d, "X.npz"), factors=X, embedding=X[:, :2].copy())
    bad = X.copy()
    bad[5, 1] = np.nan
    np.save(os.path.join(d, "Xnan.npy"), bad)
    np.save(os.path.join(d, "X1d.npy"), X[:, 0].copy())
    np.save(os.path.join(d, "blob.npy"), rs.standard_normal((40, 3)).astype(np.float32))
    np.save(os.path.join(d, "truth.npy"), truth.astype(np.int64))
    np.save(os.path.join(d, "truth_short.npy"), truth[:-1].astype(np.int64))
    np.save(os.path.join(d, "truth_float.npy"), truth.astype(np.float64))
    np.save(os.path.join(d, "blob_truth.npy"), (np.arange(40) % 2).astype(np.int64))
    np.save(os.path.join(d, "labels.npy"), truth.astype(np.int64))
    np.save(os.path.join(d, "centers.npy"), centres[:, :dim])
    np.save(os.path.join(d, "stack.npy"), rs.standard_normal((n, 8, 8)).astype(np.float32))
    order = rs.permutation(n)
    rows = np.stack([order, rs.uniform(0, 360, n), rs.uniform(-2, 2, n), rs.uniform(-2, 2, n), rs.randint(0, 2, n), truth[order]], 1)
    np.savetxt(os.path.join(d, "params.txt"), rows, fmt="%d %.4f %.4f %.4f %d %d")
    np.savetxt(os.path.join(d, "params_short.txt"), rows[:-1], fmt="%d %.4f %.4f %.4f %d %d")
    dup = rows.copy()
    dup[3, 0] = dup[4, 0]
    np.savetxt(os.path.join(d, "params_badidx.txt"), dup, fmt="%d %.4f %.4f %.4f %d %d")
    np.savetxt(os.path.join(d, "params5.txt"), rows[:, :5], fmt="%d %.4f %.4f %.4f %d")
    with open(os.path.join(d, "notnumbers.txt"), "w") as f:
        f.write("a b c\n")


SHARED = [
    ("npy", ["X.npy"], []),
    ("npz", ["X.npz"], ["--key", "factors"]),
    ("npz_embedding", ["X.npz"], ["--key", "embedding"]),
    ("npz_nokey", ["X.npz"], ["--key", "nope"]),
    ("missing_file", ["absent.npy"], []),
    ("nan", ["Xnan.npy"], []),
    ("one_d", ["X1d.npy"], []),
]
TRUTH = [
    ("truth_npy", ["--truth", "truth.npy"]),
    ("truth_params", ["--truth", "params.txt"]),
    ("truth_short_npy", ["--truth", "truth_short.npy"]),
    ("truth_float_npy", ["--truth", "truth_float.npy"]),
    ("truth_short_params", ["--truth", "params_short.txt"]),
    ("truth_badidx", ["--truth", "params_badidx.txt"]),
    ("truth_five_columns", ["--truth", "params5.txt"]),
    ("truth_not_numbers", ["--truth", "notnumbers.txt"]),
    ("truth_missing", ["--truth", "absent.txt"]),
    ("averages_no_stack", ["--averages", "refs.npy"]),
    ("averages_no_gpu", ["--averages", "refs.npy", "--stack", "stack.npy", "--params", "params.txt", "--ou", "3"]),
]


def cases():
    out = []
    own = {"kmeans": ["--k", "3", "--seed", "0"], "gmm": ["--k", "3", "--seed", "0"], "dbscan": ["--eps", "1.6"],
           "hdbscan": ["--min_cluster_size", "10"], "tsne": ["--perplexity", "10", "--max_iter", "300", "--seed", "3"]}
    for tool, base in own.items():
        for name, inp, extra in SHARED:
            out.append(("%s/%s" % (tool, name), tool, inp, base + extra))
        if tool != "tsne":
            for name, extra in TRUTH:
                out.append(("%s/%s" % (tool, name), tool, ["X.npy"], base + extra))
    out += [
        ("tsne/init_random", "tsne", ["X.npy"], own["tsne"] + ["--init", "random"]),
        ("tsne/bad_perplexity", "tsne", ["X.npy"], ["--perplexity", "500"]),
        ("kmeans/no_k", "kmeans", ["X.npy"], []),
        ("kmeans/scores_truth", "kmeans", ["X.npy"], own["kmeans"] + ["--scores", "--truth", "truth.npy"]),
        ("kmeans/sweep", "kmeans", ["X.npy"], ["--sweep", "2:4", "--seed", "1", "--sample_size", "100"]),
        ("kmeans/init_random", "kmeans", ["X.npy"], own["kmeans"] + ["--init", "random", "--n_init", "3"]),
        ("kmeans/init_file", "kmeans", ["X.npy"], own["kmeans"] + ["--init", "centers.npy"]),
        ("kmeans/k_too_large", "kmeans", ["X.npy"], ["--k", "999"]),
        ("gmm/diag_min_proba", "gmm", ["X.npy"], own["gmm"] + ["--cov", "diag", "--min_proba", "0.9", "--truth", "params.txt"]),
        ("gmm/sweep", "gmm", ["X.npy"], ["--sweep", "2,3", "--seed", "1"]),
        ("gmm/init_labels", "gmm", ["X.npy"], own["gmm"] + ["--init", "labels.npy"]),
        ("gmm/init_random", "gmm", ["X.npy"], own["gmm"] + ["--init", "random", "--n_init", "2"]),
        ("gmm/k_too_large", "gmm", ["X.npy"], ["--k", "999"]),
        ("dbscan/kdist_only", "dbscan", ["X.npy"], ["--kdist"]),
        ("dbscan/kdist_eps", "dbscan", ["X.npy"], ["--kdist", "--eps", "1.6", "--min_samples", "4"]),
        ("dbscan/no_eps", "dbscan", ["X.npy"], []),
        ("dbscan/averages_no_eps", "dbscan", ["X.npy"], ["--kdist", "--averages", "refs.npy", "--stack", "stack.npy", "--params", "params.txt",
                                                         "--ou", "3"]),
        ("dbscan/all_noise_truth", "dbscan", ["X.npy"], ["--eps", "0.001", "--truth", "truth.npy"]),
        ("dbscan/some_noise_truth", "dbscan", ["X.npy"], ["--eps", "1.2", "--min_samples", "6", "--truth", "params.txt"]),
        ("dbscan/bad_min_samples", "dbscan", ["X.npy"], ["--eps", "1.0", "--min_samples", "0"]),
        ("hdbscan/all_noise_truth", "hdbscan", ["blob.npy"], ["--min_cluster_size", "30", "--truth", "blob_truth.npy"]),
        ("hdbscan/some_noise_truth", "hdbscan", ["X.npy"], ["--min_cluster_size", "8", "--min_samples", "4", "--truth", "params.txt",
                                                            "--min_proba", "0.5"]),
        ("hdbscan/leaf", "hdbscan", ["X.npy"], ["--method", "leaf"]),
        ("hdbscan/min_cluster_size_too_large", "hdbscan", ["blob.npy"], ["--min_cluster_size", "50"]),
        ("sdr/no_gpu", "sdr", ["stack.npy"], ["--p0", "3", "--q0", "3", "--r", "4"]),
        ("sdr/params", "sdr", ["stack.npy"], ["--p0", "3", "--q0", "3", "--r", "4", "--params", "params.txt"]),
    ]
    return out


def digest(path):
    if not os.path.exists(path):
        return None
    with np.load(path) as z:
        return {k: [str(z[k].dtype), list(z[k].shape), hashlib.sha256(np.ascontiguousarray(z[k]).tobytes()).hexdigest()] for k in sorted(z.files)}


def run_all():
    env = dict(os.environ, PYTHONPATH=ROOT, PYTHONHASHSEED="0", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    listing = {}
    for name, tool, inp, opts in cases():
        with tempfile.TemporaryDirectory() as d:
            make_inputs(d)
            tail = opts if tool == "sdr" else opts + ["--backend", "numpy"]
            p = subprocess.run([sys.executable, "-m", "cryo_ralib_amd." + tool] + inp + ["out.npz"] + tail, cwd=d, env=env,
                               capture_output=True, text=True)
            mask = lambda s: re.sub(r"\.py:\d+:", ".py:N:", s)
            listing[name] = {"argv": [tool] + inp + ["out.npz"] + tail, "exit": p.returncode, "stdout": p.stdout, "stderr": mask(p.stderr),
                             "npz": digest(os.path.join(d, "out.npz")),
                             "files": sorted(f for f in os.listdir(d) if f.startswith(("out", "refs")))}
    return listing


def main(argv):
    if len(argv) == 3 and argv[0] == "--diff":
        a, b = (json.load(open(p)) for p in argv[1:])
        bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        for k in bad:
            print("differs: %s\n  %s\n  %s" % (k, json.dumps(a.get(k))[:2000], json.dumps(b.get(k))[:2000]))
        return 1 if bad else 0
    if len(argv) != 1:
        raise SystemExit(__doc__)
    listing = run_all()
    with open(argv[0], "w") as f:
        json.dump(listing, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d cases" % (argv[0], len(listing)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
