"""Shared by the CPU and GPU tests of the allocation sampler's split-merge move: the host build of the spec's stream-18
draws and of as_log_prior (tests/alloc_split/alloc_split_host.cpp), plain or under the sanitizers."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
INC = os.path.join(HERE, "..", "bmm-mcmc_amd", "csrc")
SRC = os.path.join(HERE, "alloc_split", "alloc_split_host.cpp")


def build_host(tmp_dir, sanitize=False):
    exe = os.path.join(str(tmp_dir), "alloc_split_host_san" if sanitize else "alloc_split_host")
    if not os.path.exists(exe):
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I", INC, SRC, "-o", exe], check=True)
    return exe


def _run(exe, mode, lines, tmp_dir):
    fin, fout = os.path.join(str(tmp_dir), mode + "_in.txt"), os.path.join(str(tmp_dir), mode + "_out.txt")
    with open(fin, "w") as f:
        f.write("".join(line + "\n" for line in lines))
    subprocess.run([exe, mode, fin, fout], check=True)
    with open(fout) as f:
        return [ln.split() for ln in f.read().splitlines()]


def _bits(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def host_draws(exe, tmp_dir, keys):
    """as_move_draws on the host for (seed, sweep, move, N): (i, j, the bits of u, salt) per key"""
    rows = _run(exe, "draws", ["%d %d %d %d" % k for k in keys], tmp_dir)
    assert len(rows) == len(keys)
    return [tuple(int(v) for v in r) for r in rows]


def host_prior(exe, tmp_dir, args, a, log_prior_k):
    """the bits of as_log_prior on the host for (K, N, n, n0, n1, split) tuples"""
    lp = " ".join(str(_bits(v)) for v in log_prior_k)
    lines = ["%d %d %d %d %d %d %d %d %s" % (K, N, _bits(a), n, n0, n1, int(split), len(log_prior_k), lp) for K, N, n, n0, n1, split in args]
    rows = _run(exe, "prior", lines, tmp_dir)
    assert len(rows) == len(args)
    return np.array([int(r[0]) for r in rows], dtype=np.uint64)
