"""numpy restatement of mmc_batch_structure_factor for the structure-factor tests (not a test
module): the definitions of include/mmc_hip.h, "Partial structure factors", operation by operation
in unfused fp64, so that the device (built with -ffp-contract=off) can be asked to agree BIT FOR
BIT.  Nothing is left unrestated:

  phase factors   (cos, sin) of (MMC_TWOPI x) / L by sincos_moderate, both from
                  tests/elementary_ref.py (its fma is exact; both argument branches), one scalar
                  call per coordinate (phase_factors);
  powers          p_0 = 1, p_k = c_mul(p_{k-1}, e1): sq_pow's first product is 1 e1, which is
                  exact, and a block's first power z1^k0 is the same k0 products from 1;
  negative ny     the conjugate of y1^|ny|, taken after the power;
  the term        c_mul(c_mul(ex, ey), p_k) for nz = k, c_mul(c_mul(ex, ey), conj(p_k)) for nz = -k;
  the sums        lane l of 64 adds the molecules l, l + 64, ... in that order from 0.0, the 64 lane
                  sums go through wave_sum's tree (lane_sum);
  a row's value   re_a re_b + im_a im_b: two products and one add;
  Q               v 2^24 (exact) rounded to the nearest integer, ties to even -- the device's
                  1.5 2^52 add; np.rint rounds the same way -- and the doubling of the half space.

sofq_rows_direct is a second, independent form: np.longdouble, cos and sin of 2 pi n . r / L taken
directly, plain sums."""
import numpy as np

import elementary_ref as er

SCALE = 2.0 ** 24
SLOT_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def shell_counts(n_max):
    """int64 [n_max^2 + 1]: the integer vectors n with |n|^2 = s, 0 for s = 0 (brute force)."""
    out = np.zeros(n_max * n_max + 1, dtype=np.int64)
    for nx in range(-n_max, n_max + 1):
        for ny in range(-n_max, n_max + 1):
            for nz in range(-n_max, n_max + 1):
                s = nx * nx + ny * ny + nz * nz
                if 0 < s <= n_max * n_max:
                    out[s] += 1
    return out


def half_space_columns(n_max):
    """[(nx, ny, [nz ...])] of the half space nx > 0, or nx = 0 and ny > 0, or nx = ny = 0 and
    nz > 0, with 0 < |n|^2 <= n_max^2."""
    cols = []
    for nx in range(0, n_max + 1):
        for ny in range(-n_max, n_max + 1):
            if nx == 0 and ny < 0:
                continue
            rem = n_max * n_max - nx * nx - ny * ny
            if rem < 0:
                continue
            m = int(np.floor(np.sqrt(rem)))
            while (m + 1) * (m + 1) <= rem:
                m += 1
            while m * m > rem:
                m -= 1
            nz = [k for k in range(-m, m + 1) if nx > 0 or ny > 0 or k > 0]
            if nz:
                cols.append((nx, ny, nz))
    return cols


def c_mul(a, b):
    """(re, im) of the unfused complex product (csrc/mmc_device.hpp: c_mul)."""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def powers(e1, n_max):
    """[p_0 .. p_n_max] with p_0 = 1 and p_k = c_mul(p_{k-1}, e1)."""
    p = [(np.ones_like(e1[0]), np.zeros_like(e1[0]))]
    for _ in range(n_max):
        p.append(c_mul(p[-1], e1))
    return p


def lane_sum(t):
    """t [..., N]: lane l of 64 adds entries l, l + 64, ... in that order from 0.0, then wave_sum's
    tree (lane l += lane l + 32, 16, 8, 4, 2, 1): what lane 0 holds."""
    n = t.shape[-1]
    k = -(-n // 64)
    pad = np.zeros(t.shape[:-1] + (64 * k,), dtype=np.float64)
    pad[..., :n] = t
    pad = pad.reshape(t.shape[:-1] + (k, 64))
    acc = np.zeros(t.shape[:-1] + (64,), dtype=np.float64)
    for j in range(k):
        acc = acc + pad[..., j, :]
    off = 32
    while off >= 1:
        acc = acc[..., :off] + acc[..., off:2 * off]
        off //= 2
    return acc[..., 0]


def quant(v):
    """Q(v): v 2^24 rounded to the nearest integer, ties to even, int64."""
    return np.rint(np.asarray(v, dtype=np.float64) * SCALE).astype(np.int64)


def _slots(coords):
    c = np.asarray(coords, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] % 3:
        raise ValueError("coords: [3 N, 3], the atoms of a molecule together")
    return c.reshape(-1, 3, 3).transpose(1, 0, 2)     # [slot, molecule, component]


def phase_factors(coords, box):
    """[(re, im)] for the axes x, y, z, each float64 [slot, molecule]: elementary_ref.phase of every
    coordinate -- the device's sincos_moderate at the device's argument, one scalar call each."""
    x = _slots(coords)
    L = float(box)
    ph = np.array([er.phase(float(v), L) for v in x.ravel()], dtype=np.float64).reshape(x.shape + (2,))
    return [(ph[..., d, 0].copy(), ph[..., d, 1].copy()) for d in range(3)]


def sofq_rows(coords, box, n_max):
    """int64 [6, n_max^2 + 1] of one frame of 3-site molecules (coords [3 N, 3]) in a box of side
    `box`: sq[row][s] = 2 sum over the half-space vectors of shell s of Q(rho_a.re rho_b.re +
    rho_a.im rho_b.im)."""
    px, py, pz = (powers(e, n_max) for e in phase_factors(coords, box))
    out = np.zeros((6, n_max * n_max + 1), dtype=np.int64)
    for nx, ny, nzs in half_space_columns(n_max):
        ex, ey = px[nx], py[abs(ny)]
        if ny < 0:
            ey = (ey[0], -ey[1])
        xy = c_mul(ex, ey)
        nz = np.asarray(nzs)
        ez_re = np.stack([pz[abs(k)][0] for k in nzs])                        # [nz, slot, molecule]
        ez_im = np.stack([pz[abs(k)][1] if k >= 0 else -pz[abs(k)][1] for k in nzs])
        t = c_mul((xy[0][None], xy[1][None]), (ez_re, ez_im))
        re, im = lane_sum(t[0]), lane_sum(t[1])                               # [nz, slot]
        s = nx * nx + ny * ny + nz * nz
        for row, (a, b) in enumerate(SLOT_PAIRS):
            np.add.at(out[row], s, 2 * quant(re[:, a] * re[:, b] + im[:, a] * im[:, b]))
    return out


def sofq_rows_direct(coords, box, n_max):
    """The same rows by the independent form: extended precision, the phase 2 pi n . r / L of every
    atom and vector taken directly."""
    ld = np.longdouble
    x = _slots(coords).astype(ld)
    twopi_l = 2 * np.arctan2(ld(0), ld(-1)) / ld(box)
    out = np.zeros((6, n_max * n_max + 1), dtype=np.int64)
    for nx, ny, nzs in half_space_columns(n_max):
        nz = np.asarray(nzs)
        base = ld(nx) * x[..., 0] + ld(ny) * x[..., 1]                        # [slot, molecule]
        ang = twopi_l * (base[None] + nz.astype(ld)[:, None, None] * x[..., 2][None])
        re, im = np.cos(ang).sum(-1), np.sin(ang).sum(-1)                      # [nz, slot]
        s = nx * nx + ny * ny + nz * nz
        for row, (a, b) in enumerate(SLOT_PAIRS):
            v = re[:, a] * re[:, b] + im[:, a] * im[:, b]
            np.add.at(out[row], s, 2 * np.rint(v * ld(SCALE)).astype(np.int64))
    return out


def random_molecules(n_mol, box, seed):
    """coords [3 N, 3]: random rigid-ish 3-site molecules (site 0 anywhere in the box, sites 1 and 2
    about 1 A away), not wrapped."""
    rng = np.random.default_rng(seed)
    c0 = rng.random((n_mol, 1, 3)) * box
    d = rng.normal(size=(n_mol, 2, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.concatenate([c0, c0 + d], axis=1).reshape(-1, 3)
