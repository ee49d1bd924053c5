#!/usr/bin/env python3
"""Writes lar_long.npz next to this script: the 50-digit restatement of the latent autoregressive engine's iteration (tests/lar_mp.py `run`, banded
form) on every case of lar_mp.GRID and lar_mp.SCAN, as float64.  Prints its own runtime (the two T = 4096 engines are most of it).  Run from the
repo root:
    python tests/golden/make_lar_long_golden.py

Stored, in the order of GRID + SCAN:
    values   one float64 vector: per case what lar_mp.pick keeps, one case after the other; `lar_mp.errors` reads a case's slice back
    sizes    the length of every case's slice
    crc      CRC-32 of every case's inputs (lar_mp.checksum): the inputs are not stored but regenerated from the spec
    gauges   per case (largest |m_i|/sd_i, smallest R/Szz, largest cond Λ) over all iterations: the envelope's gauges, from the 50-digit run
The file has to stay below the largest fixture there was before it (76 773 bytes), so lar_mp.pick keeps a stated subset: θ's mean and variances, b
and F of every iteration, θ's whole covariance, a and the per-series F of the last; of the states, of ONE series (the first; at T = 4096 the one with
the 200 missing steps; of a shared batch the series 0, 63, 64 and the last), q(x[t]) in full at t = 1, p + 1 and T (the scan: 1 and T) and q(z_t) at
every 16th step and the last (T ≤ 64), every 32nd (T = 257), every 256th (T = 4096).  The free energy of every case is asserted non-increasing on the 50-digit values before they are rounded.  The
output is a plain (uncompressed) npz with a fixed member order: two runs give the same bytes."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "lar_long.npz")
LIMIT = 76773


def main():
    sys.path.insert(0, os.path.join(HERE, ".."))
    import lar_mp as MP

    start = time.time()
    values, sizes, crc, gauges = [], [], [], []
    for spec in MP.GRID + MP.SCAN:
        y, m, iters, share = MP.case(spec)
        crc.append(MP.checksum(y, m))
        r = MP.run(y, m, iters, share)
        assert all(b <= a for a, b in zip(r["fe_mp"], r["fe_mp"][1:])), (spec.name, r["fe"])
        v = MP.flatten(MP.pick(spec, r))
        assert np.all(np.isfinite(v)), spec.name
        values.append(v)
        sizes.append(v.size)
        gauges.append(r["gauges"])
        print(f"{spec.name}: {v.size} values, F = {r['fe'][-1]!r}, |m|/sd ≤ {r['gauges'][0]:.3g}, R/Szz ≥ {r['gauges'][1]:.3g}, cond Λ ≤ {r['gauges'][2]:.3g}", flush=True)
    np.savez(OUT, values=np.concatenate(values), sizes=np.array(sizes, dtype=np.int32), crc=np.array(crc, dtype=np.uint32), gauges=np.array(gauges))
    n = os.path.getsize(OUT)
    print(f"{OUT}: {n} bytes, {sum(sizes)} values, {time.time() - start:.0f} s")
    assert n < LIMIT, n


if __name__ == "__main__":
    main()
