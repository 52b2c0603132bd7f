"""numpy restatement of mmc_batch_cavity / mmc_batch_cavity_at (include/mmc_hip.h, "Cavities and
occupancy") for the cavity tests (not a test module).  From coordinates and points alone, in
exactly the arithmetic the header states: vector1D images per component, r^2 = (dx dx + dy dy) + dz dz
unfused, strict r^2 < R_k R_k, the nearest site under the key (bits of r^2, index), and
searchsorted(e2, r2, side="right") - 1 for its bin."""
import numpy as np

from structure_ref import vector1d


def sites_of(com, coords, site):
    """[N, 3]: atom slot `site` of every 3-atom molecule, or the centres of mass for site = -1."""
    if site == -1:
        return np.asarray(com, dtype=np.float64)
    if site not in (0, 1, 2):
        raise ValueError("site must be -1, 0, 1 or 2")
    return np.asarray(coords, dtype=np.float64)[site::3]


def distances2(points, sites, box):
    """r^2 [P, N] of d = vector1D(point, site)."""
    d = vector1d(np.asarray(points, dtype=np.float64)[:, None, :], np.asarray(sites, dtype=np.float64)[None, :, :], box)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nn_edges2(nn_bins, nn_max):
    """e2[m] = (m dr)(m dr), m = 0 .. nn_bins, dr = nn_max / nn_bins."""
    dr = np.float64(nn_max) / np.float64(nn_bins)
    e = np.arange(nn_bins + 1, dtype=np.float64) * dr
    return e * e


def nn_bin(r2, nn_bins, nn_max):
    return np.searchsorted(nn_edges2(nn_bins, nn_max), r2, side="right") - 1


def cavity(sites, points, box, radii, n_cap, nn_bins=0, nn_max=None):
    """Everything the call returns for one replica: dict with count int32 [P, K], nn_r2 [P], nn_idx
    int32 [P], occ_hist uint64 [K, n_cap + 1], occ_mom uint64 [K, 2] and, with nn_bins > 0, nn_hist
    uint64 [nn_bins + 1]."""
    radii = np.asarray(radii, dtype=np.float64)
    r2 = distances2(points, sites, box)
    count = np.stack([(r2 < R * R).sum(1) for R in radii], axis=1).astype(np.int32)
    bits = np.ascontiguousarray(r2).view(np.uint64)
    idx = np.argmin(bits, axis=1).astype(np.int32)            # the first of equal keys: the lower index
    nn_r2 = r2[np.arange(r2.shape[0]), idx]
    K = radii.shape[0]
    occ_hist = np.stack([np.bincount(np.minimum(count[:, k], n_cap), minlength=n_cap + 1) for k in range(K)]).astype(np.uint64)
    c = count.astype(np.uint64)
    occ_mom = np.stack([c.sum(0), (c * c).sum(0)], axis=1).astype(np.uint64)
    out = dict(count=count, nn_r2=nn_r2, nn_idx=idx, occ_hist=occ_hist, occ_mom=occ_mom)
    if nn_bins > 0:
        out["nn_hist"] = np.bincount(nn_bin(nn_r2, nn_bins, nn_max), minlength=nn_bins + 1).astype(np.uint64)
    return out
