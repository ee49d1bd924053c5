#!/usr/bin/env python3
"""Writes hmm_long.npz next to this script: the 50-digit restatement of the hidden Markov model engine's iteration (tests/hmm_mp.py `run`) on
every case of hmm_mp.GRID and hmm_mp.SCAN, as float64.  About a minute (the two T = 4096 chains are most of it).  Run from the repo root:
    python tests/golden/make_hmm_long_golden.py

Stored, in the order of GRID + SCAN:
    values   one float64 vector: per case what hmm_mp.pick keeps (a stated subset: the file has to stay below the largest fixture there was before
             it, 50 272 bytes), one case after the other; `hmm_mp.errors` reads a case's slice back
    sizes    the length of every case's slice (0: not stored, see below)
    crc      CRC-32 of every case's inputs (hmm_mp.checksum): the inputs are not stored but regenerated from the spec
A scan case whose smallest normaliser in the DOUBLE restatement (hmm_ref.min_normaliser) is at or below hmm_ref.K_MIN_NORMALISER / 10 has to be
refused by the engine, so no answer is stored for it.  The output is a plain (uncompressed) npz with a fixed member order: two runs give the
same bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "hmm_long.npz")
LIMIT = 50272


def must_be_refused(R, x, m, iterations):
    return R.min_normaliser(x, **m, iterations=iterations) <= R.K_MIN_NORMALISER / 10


def main():
    sys.path.insert(0, os.path.join(HERE, ".."))
    import hmm_mp as MP
    import hmm_ref as R

    values, sizes, crc = [], [], []
    for spec in MP.GRID + MP.SCAN:
        x, m = MP.case(spec)
        crc.append(MP.checksum(x, m))
        if spec in MP.SCAN and must_be_refused(R, x, m, spec.iterations):
            sizes.append(0)
            continue
        r = MP.run(x, **m, iterations=spec.iterations, share=spec.share)
        v = MP.flatten(MP.pick(spec, r["gamma"][-1], r["A"][-1], r["B"][-1], r["fe"]))
        assert np.all(np.isfinite(v)), spec.name
        values.append(v)
        sizes.append(v.size)
        print(f"{spec.name}: {v.size} values, F = {r['fe'][-1]!r}, log10 of the smallest normaliser {min(r['log10_normaliser']):.1f}")
    np.savez(OUT, values=np.concatenate(values), sizes=np.array(sizes, dtype=np.int16), crc=np.array(crc, dtype=np.uint32))
    n = os.path.getsize(OUT)
    print(f"{OUT}: {n} bytes, {sum(sizes)} values, {sizes.count(0)} scan cases not stored")
    assert n < LIMIT, n


if __name__ == "__main__":
    main()
