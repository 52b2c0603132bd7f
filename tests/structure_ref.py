"""numpy restatement of mmc_batch_rdf_sites and mmc_batch_dipoles for the structure tests (not a
test module).  The pair loop is oracle/numpy_check.make_rdf_hist's (Ewald/gr.jl:60-91) with the bin
width a parameter and a second site array for the cross rows."""
import numpy as np

from metropolismontecarlo_amd.observables import SLOT_PAIRS


def pair_hist(A, B, side, dr, numbins):
    """Counts of A[i] - B[j]: over i < j when B is None (A against itself), else over all ordered
    i != j.  gr.jl's image (strict < -side/2 -> + side, > side/2 -> - side),
    r = sqrt((xx xx + yy yy) + zz zz), bin = ceil(r / dr), counted when bin <= numbins."""
    A = np.asarray(A, dtype=np.float64)
    sideh = side / 2.0
    hist = np.zeros(numbins + 1, dtype=np.uint64)
    n = A.shape[0]
    for i in range(n):
        other = A[i + 1:] if B is None else np.delete(np.asarray(B, dtype=np.float64), i, axis=0)
        if other.shape[0] == 0:
            continue
        d = A[i] - other
        d = np.where(d < -sideh, d + side, d)
        d = np.where(d > sideh, d - side, d)
        rij = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        b = np.ceil(rij / dr)
        b = b[b <= numbins].astype(np.int64)
        np.add.at(hist, b, 1)
    return hist


def six_rows(coords, side, numbins, r_max=0.0):
    """[6, numbins + 1]: the rows of SLOT_PAIRS for one frame of 3-site molecules, coords [3 N, 3]."""
    coords = np.asarray(coords, dtype=np.float64)
    dr = (side / 2.0) / numbins if r_max <= 0 else r_max / numbins
    return np.stack([pair_hist(coords[a::3], None if a == b else coords[b::3], side, dr, numbins)
                     for a, b in SLOT_PAIRS])


def vector1d(c1, c2, box):
    """Ewald/boundaries.jl vector1D as csrc/mmc_device.hpp states it: d = c2 - c1, moved by one box
    when |d| >= box / 2."""
    d = np.asarray(c2, dtype=np.float64) - np.asarray(c1, dtype=np.float64)
    m = np.where(np.abs(d) < 0.5 * box, 0.0, np.copysign(1.0, d))
    return d - m * box


def molecule_dipoles(com, coords, charge, box):
    """mu_i [N, 3] = (q_0 d_0 + q_1 d_1) + q_2 d_2, d_a = vector1D(COM, atom a)."""
    com, coords = np.asarray(com, dtype=np.float64), np.asarray(coords, dtype=np.float64)
    q = np.asarray(charge, dtype=np.float64)
    d = [vector1d(com, coords[a::3], box) for a in range(3)]
    return (q[0::3, None] * d[0] + q[1::3, None] * d[1]) + q[2::3, None] * d[2]
