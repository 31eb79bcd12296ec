#!/usr/bin/env python3
"""Generate tests/golden/edit_ref.npz from the REFERENCE'S OWN ``ctc_fast/editDistance.py``
(DESIGN.md §4.8).

The unmodified file of the reference checkout is copied into a scratch directory OUTSIDE the
repository, its tabs expanded (``expand -t 8``: it mixes tabs and spaces, which Python 3
refuses) and converted with ``lib2to3`` (``xrange``, ``print``); the converted module is
imported from there and run on every pair.  Only inputs and the five results are stored.

Pairs: the reference's own two examples and the two one-sided cases, empty against empty, and
seeded random pairs of lengths 0..40 over alphabets of 2, 3, 5 and 30 symbols
(tests/edit_model.random_pairs: half of the hypotheses are edits of their reference).

  edit_ref.npz   a, b       int32, all sequences concatenated
                 a_len, b_len   int32 [P]
                 result     float64 [P][5]: dist, ins, dels, subs, corr of
                            editDistance.edit_distance(ref = a, hyp = b)

``swbd-utils/editDist.pyx`` is not run: the installed Cython rejects its ``np.int_t``
declarations (tests/edit_model.py restates it instead).

Usage:  python tests/golden/make_golden_edit.py --reference <reference checkout> [--scratch DIR] [--out DIR]
"""
import argparse
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import edit_model  # noqa: E402

LITERAL = [("saturday", "sunday"), ("kitten", "sitting"), ("", "ab"), ("ab", ""), ("", "")]


def load_reference(reference, scratch):
    src = os.path.join(reference, "ctc_fast", "editDistance.py")
    dst = os.path.join(scratch, "editDistance_ref.py")
    with open(dst, "wb") as f:
        f.write(subprocess.check_output(["expand", "-t", "8", src]))
    subprocess.check_call([sys.executable, "-m", "lib2to3", "-w", "-n", dst], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    spec = importlib.util.spec_from_file_location("editDistance_ref", dst)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    out = [(np.array([ord(c) for c in a], dtype=np.int32), np.array([ord(c) for c in b], dtype=np.int32))
           for a, b in LITERAL]
    out += edit_model.random_pairs(20240, 400, 40, [2, 3, 5, 30])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True)
    ap.add_argument("--scratch")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    scratch = a.scratch or tempfile.mkdtemp(prefix="edit_ref_")
    if os.path.commonpath([os.path.abspath(scratch), ROOT]) == ROOT:
        ap.error("the scratch directory must lie outside the repository")
    os.makedirs(scratch, exist_ok=True)
    ref = load_reference(a.reference, scratch)
    pairs = cases()
    res = np.zeros((len(pairs), 5), dtype=np.float64)
    for p, (x, y) in enumerate(pairs):
        res[p] = ref.edit_distance(list(x), list(y))
    np.savez_compressed(os.path.join(a.out, "edit_ref.npz"),
                        a=np.concatenate([x for x, _ in pairs]).astype(np.int32),
                        b=np.concatenate([y for _, y in pairs]).astype(np.int32),
                        a_len=np.array([len(x) for x, _ in pairs], dtype=np.int32),
                        b_len=np.array([len(y) for _, y in pairs], dtype=np.int32), result=res)
    if not a.scratch:
        shutil.rmtree(scratch, ignore_errors=True)
    print("wrote %d pairs to %s" % (len(pairs), os.path.join(a.out, "edit_ref.npz")))


if __name__ == "__main__":
    main()
