"""numpy restatement of mmc_batch_shell_order (include/mmc_hip.h, "Shell order") for the shell-order
tests (not a test module): every molecule's O-O neighbours inside r_list sorted under (bits of r^2,
j), the rank histograms, the local structure index, zeta and the O-O-O angles, in exactly the
arithmetic the header states -- vector1D images per component, every r^2 and dot product
(x x' + y y') + z z' unfused, the serial sums as explicit loops in rising k -- and the frames that
the CPU and the GPU tests share."""
import numpy as np

import common
from local_order_ref import cubic_lattice, dot3, frame, hbond_matrix, oo_vectors, water
from structure_ref import vector1d

CAP = 64        # MMC_SHELL_CAP
NBR = 16        # MMC_SHELL_NBR
DEFAULTS = dict(r_list=6.0, r_lsi=3.7, r_ang=3.3, r_hb=3.5, theta_deg=30.0, n_rank=8, r_bins=300, lsi_bins=200,
                lsi_max=0.4, ang_bins=180, zeta_bins=200, zeta_lo=-1.5, zeta_hi=2.5)


def params(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def clamp_bin(x, top):
    """(int)floor(x) clamped to 0 .. top, the clamps made on the double (x finite or +-inf)."""
    return int(min(max(np.floor(x), 0.0), float(top)))


def serial_sum(terms):
    s = terms[0]
    for t in terms[1:]:
        s = s + t
    return s


def lsi_of(rho, n):
    """I of the header from the sorted distances: n >= 1 gaps rho[k + 1] - rho[k], k < n."""
    delta = [rho[k + 1] - rho[k] for k in range(n)]
    mean = serial_sum(delta) / np.float64(n)
    return serial_sum([(dk - mean) * (dk - mean) for dk in delta]) / np.float64(n)


def shell_order(coords, box, r_list=6.0, r_lsi=3.7, r_ang=3.3, r_hb=3.5, theta_deg=30.0, n_rank=8, r_bins=300,
                lsi_bins=200, lsi_max=0.4, ang_bins=180, zeta_bins=200, zeta_lo=-1.5, zeta_hi=2.5):
    """Everything the call returns for one replica, and what the tests ask about the frame: dict with
    count [N] int32, nbr [N, 16] int32, lsi [N], zeta [N], rank_hist [n_rank, r_bins + 1], lsi_hist,
    ang_hist, zeta_hist (uint64), flagged (int), and per molecule n_lsi, m_ang, n_bonded (int64, -1
    where flagged), ties (bool: two listed neighbours with equal r^2 bits)."""
    box = np.float64(box)
    cos_hb = np.float64(np.cos(np.deg2rad(float(theta_deg))))
    d, r2 = oo_vectors(coords, box)
    n_mol = r2.shape[0]
    bits = np.ascontiguousarray(r2).view(np.uint64)
    B = hbond_matrix(coords, box, r_hb, cos_hb).any(axis=1)        # [donor, acceptor]
    bonded = B | B.T
    rl2, rlsi2, rang2 = np.float64(r_list) * r_list, np.float64(r_lsi) * r_lsi, np.float64(r_ang) * r_ang
    inv_dr, lsi_scale = r_bins / np.float64(r_list), lsi_bins / np.float64(lsi_max)
    ang_scale, zeta_scale = ang_bins / 2.0, zeta_bins / (np.float64(zeta_hi) - np.float64(zeta_lo))

    out = dict(count=np.full(n_mol, -1, np.int32), nbr=np.full((n_mol, NBR), -1, np.int32),
               lsi=np.full(n_mol, np.nan), zeta=np.full(n_mol, np.nan),
               rank_hist=np.zeros((n_rank, r_bins + 1), np.uint64), lsi_hist=np.zeros(lsi_bins + 1, np.uint64),
               ang_hist=np.zeros(ang_bins + 1, np.uint64), zeta_hist=np.zeros(zeta_bins + 1, np.uint64), flagged=0,
               n_lsi=np.full(n_mol, -1, np.int64), m_ang=np.full(n_mol, -1, np.int64),
               n_bonded=np.full(n_mol, -1, np.int64), ties=np.zeros(n_mol, bool))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n_mol):
            js = np.flatnonzero(r2[i] < rl2)
            js = js[js != i]
            m = len(js)
            if m > CAP:
                out["flagged"] += 1
                continue
            lst = js[np.lexsort((js, bits[i, js]))]                 # last key first: bits, then j
            rr = r2[i, lst]
            rho = np.sqrt(rr)
            out["count"][i] = m
            out["nbr"][i, :min(m, NBR)] = lst[:NBR]
            out["ties"][i] = m > 1 and bool(np.any(rr[1:] == rr[:-1]))
            for k in range(n_rank):
                out["rank_hist"][k, clamp_bin(rho[k] * inv_dr, r_bins - 1) if k < m else r_bins] += 1
            # LSI
            n = int(np.count_nonzero(rr < rlsi2))
            out["n_lsi"][i] = n
            if n >= 1 and m >= n + 1:
                out["lsi"][i] = lsi_of(rho, n)
                out["lsi_hist"][clamp_bin(out["lsi"][i] * lsi_scale, lsi_bins - 1)] += 1
            else:
                out["lsi_hist"][lsi_bins] += 1
            # zeta
            bd = bonded[i, lst]
            out["n_bonded"][i] = bd.sum()
            if bd.any() and not bd.all():
                out["zeta"][i] = rho[np.flatnonzero(~bd)[0]] - rho[np.flatnonzero(bd)[-1]]
                out["zeta_hist"][clamp_bin((out["zeta"][i] - np.float64(zeta_lo)) * zeta_scale, zeta_bins - 1)] += 1
            else:
                out["zeta_hist"][zeta_bins] += 1
            # angles
            ma = int(np.count_nonzero(rr < rang2))
            out["m_ang"][i] = ma
            if ma >= 2:
                ja, ka = np.triu_indices(ma, 1)
                dd = d[i, lst[:ma]]
                c = dot3(dd[ja], dd[ka]) / np.sqrt(rr[ja] * rr[ka])
                for ck in c:
                    out["ang_hist"][clamp_bin((ck + 1.0) * ang_scale, ang_bins - 1) if np.isfinite(ck) else ang_bins] += 1
    return out


def lsi_bin(v, lsi_bins, lsi_max):
    """The header's bin of every LSI value (int64; lsi_bins for NaN)."""
    scale = lsi_bins / np.float64(lsi_max)
    return np.array([clamp_bin(x * scale, lsi_bins - 1) if np.isfinite(x) else lsi_bins for x in np.ravel(v)], np.int64)


def zeta_bin(v, zeta_bins, lo, hi):
    scale = zeta_bins / (np.float64(hi) - np.float64(lo))
    return np.array([clamp_bin((x - np.float64(lo)) * scale, zeta_bins - 1) if np.isfinite(x) else zeta_bins
                     for x in np.ravel(v)], np.int64)


# ---- frames for the tests: each returns the arrays of a batch (tests/common.py) ---------------------
BOX = 22.0
SIZES = (2, 3, 64, 65, 66, 129)
# the three ranges the random frames are taken at, with bin counts 1, 7 and 1024 and n_rank 1 and 16
CASES = {
    "3.7": params(r_list=3.7, r_lsi=3.5, r_ang=3.6, r_hb=3.7, theta_deg=75.0, n_rank=1, r_bins=1024, lsi_bins=1024,
                  lsi_max=0.05, ang_bins=1024, zeta_bins=1024),
    "7": params(r_list=7.0, r_lsi=4.5, r_ang=5.0, r_hb=4.5, theta_deg=50.0, n_rank=16, r_bins=7, lsi_bins=7,
                lsi_max=0.1, ang_bins=7, zeta_bins=7, zeta_lo=-0.5, zeta_hi=1.0),
    "L/2": params(r_list=0.5 * BOX, r_lsi=6.0, r_ang=4.0, r_hb=4.0, theta_deg=60.0, n_rank=16, r_bins=1, lsi_bins=1,
                  ang_bins=1, zeta_bins=1),
}
# counters that leave a workgroup two waves (7472 words) and one (8000, the bound): the lists of four
# waves no longer fit beside them in 32 KiB
FEWER_WAVES = {
    2: params(r_list=7.0, r_lsi=4.5, r_ang=5.0, r_hb=4.5, theta_deg=50.0, n_rank=7, r_bins=1023, lsi_bins=100, lsi_max=0.1,
              ang_bins=100, zeta_bins=100),
    1: params(r_list=7.0, r_lsi=4.5, r_ang=5.0, r_hb=4.5, theta_deg=50.0, n_rank=7, r_bins=1023, lsi_bins=276, lsi_max=0.1,
              ang_bins=276, zeta_bins=276),
}


def lattice_params(a):
    """On a simple-cubic lattice of spacing a: a < r_ang = r_hb < r_lsi < a sqrt(2) < r_list < a sqrt(3)."""
    return params(r_list=1.55 * a, r_lsi=1.2 * a, r_ang=1.1 * a, r_hb=1.1 * a, lsi_max=1.0)


def random_frame(n_mol, seed=None):
    """Mixed atom types on a jittered lattice that fills the box from one side: the SoA path."""
    return common.random_system(n_mol, BOX, seed=700 + n_mol if seed is None else seed, na_choices=(3,))


def replica_frame(a, r):
    """(com, coords) of replica r of a batch made from the random frame `a`: r = 0 as it is, then
    other draws of the positions, every molecule moved into the box by its centre of mass."""
    if r == 0:
        return a["com"], a["coords"]
    n_mol = len(a["com"])
    o = random_frame(n_mol, seed=7000 + 100 * r + n_mol)
    sh = np.random.default_rng(r).random(3) * a["box"]
    com = (o["com"] + sh) % a["box"]
    return com, o["coords"] + np.repeat(com - o["com"], 3, axis=0)


def water_arrays(coords, box):
    """Waters with the force field of NIST configuration 1 at the given [3 N, 3] coordinates."""
    a = common.nist_arrays(1, "unwrapped")
    coords = np.asarray(coords, dtype=np.float64)
    m = len(coords) // 3
    w = np.array([15.9994, 1.008, 1.008])
    com = (coords.reshape(m, 3, 3) * w[None, :, None]).sum(1) / w.sum()
    return dict(a, com=com, coords=coords, atype=np.tile(a["atype"][:3], m), charge=np.tile(a["charge"][:3], m),
                first_atom=1 + 3 * np.arange(m, dtype=np.int64), last_atom=3 + 3 * np.arange(m, dtype=np.int64),
                box=float(box))


def lattice_frame(n, spacing):
    O, box = cubic_lattice(n, spacing)
    return water_arrays(frame(O, box), box)


def ball_frame(n_mol, diameter=5.0, seed=3):
    """n_mol oxygens inside a ball of the given diameter in the middle of the box: every one has
    all the others inside r_list >= diameter."""
    rng = np.random.default_rng(seed)
    g = np.arange(-4, 5) * 0.8
    pts = np.array([[x, y, z] for x in g for y in g for z in g])
    pts = pts[np.argsort((pts * pts).sum(1), kind="stable")][:n_mol]
    pts = pts + (rng.random(pts.shape) - 0.5) * 0.1
    assert np.sqrt((pts * pts).sum(1)).max() < 0.5 * diameter
    dirs = rng.normal(size=(n_mol, 3))
    return water_arrays(frame(list(pts + 0.5 * BOX), BOX, [list(v) for v in dirs]), BOX)


def coincident_frame(n_mol=20):
    """A random frame in which molecule 1 lies exactly on molecule 0."""
    a = random_frame(n_mol, seed=41)
    a["coords"][3:6] = a["coords"][0:3]
    a["com"][1] = a["com"][0]
    return a


PENTAMER_R, PENTAMER_FAR = 2.8, 3.4


def pentamer_frame():
    """A water with four bonded neighbours at 2.8 A on a tetrahedron -- it donates to two and accepts
    from two -- and a sixth molecule at 3.4 A that is bonded to nobody: zeta = 3.4 - 2.8."""
    c = np.full(3, 0.5 * BOX)
    t = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)
    mols = [water(c, t[0], t[1])]                                   # H towards neighbours 0 and 1
    mols += [water(c + PENTAMER_R * t[0], t[0], [0.0, 0.0, 1.0]), water(c + PENTAMER_R * t[1], t[1], [0.0, 0.0, 1.0])]
    mols += [water(c + PENTAMER_R * t[k], -t[k], [0.0, 0.0, 1.0]) for k in (2, 3)]   # these donate to the centre
    far = -t[0]                                                     # opposite a vertex: between three others
    mols.append(water(c + PENTAMER_FAR * far, far, [0.0, 0.0, 1.0]))
    return water_arrays(np.concatenate(mols), BOX)
