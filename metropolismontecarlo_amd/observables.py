"""Observables built on the device state: normalisation of the radial
distribution histogram exactly as Ewald/gr.jl:92-104 writes it."""
import numpy as np


def normalize_rdf(hist, npart, side, nstep):
    """gr.jl:92-104: phi = npart / side^3, norm = 2 pi dr phi nstep npart,
    g(r_i) = hist[i] / norm / (r_i^2 + dr^2/12) at r_i = (i - 1/2) dr, i = 1..numbins.
    `hist` has numbins + 1 entries (index 0 unused, as in gr.jl).  Returns (r, g)."""
    hist = np.asarray(hist, dtype=float)
    numbins = hist.shape[0] - 1
    dr = (side / 2.0) / numbins
    phi = npart / side ** 3
    norm = 2.0 * np.pi * dr * phi * nstep * npart
    i = np.arange(1, numbins + 1)
    rrr = (i - 0.5) * dr
    return rrr, hist[1:] / norm / (rrr * rrr + dr * dr / 12.0)


# ---- site-site pair histograms and dipole moments (include/mmc_hip.h, "Structure observables") ----
SLOT_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # rows of mmc_batch_rdf_sites, in order


def fold_by_type(hist6, slot_types):
    """Sum the rows of an mmc_batch_rdf_sites histogram ([..., 6, numbins + 1]) whose slot pairs
    have the same unordered type pair.  slot_types: the type of each of the three slots, e.g.
    ("O", "H", "H").  Returns ({(t1, t2): rows [..., numbins + 1]}, {(t1, t2): site pairs per
    molecule pair}) with t1 <= t2.  A row (a, a) holds one site pair per molecule pair, a row
    (a, b), a < b, two; SPC/E: OO = (0,0), 1; OH = (0,1) + (0,2), 4; HH = (1,1) + (1,2) + (2,2), 4."""
    hist6 = np.asarray(hist6)
    if hist6.shape[-2] != 6 or len(slot_types) != 3:
        raise ValueError("hist6 must be [..., 6, numbins + 1] and slot_types three types")
    rows, counts = {}, {}
    for k, (a, b) in enumerate(SLOT_PAIRS):
        key = tuple(sorted((slot_types[a], slot_types[b])))
        rows[key] = hist6[..., k, :] + rows[key] if key in rows else hist6[..., k, :].copy()
        counts[key] = counts.get(key, 0) + (1 if a == b else 2)
    return rows, counts


def normalize_rdf_pairs(row, n_site_pairs, dr, inv_volume_sum):
    """g(r) of one (folded) row of pair counts, row[0 .. numbins]:
    g(r_i) = row[i] / (n_site_pairs inv_volume_sum 4 pi (r_i^2 + dr^2/12) dr) at r_i = (i - 1/2) dr,
    i = 1..numbins.  n_site_pairs: the counted site pairs per frame (for N molecules N (N - 1) / 2
    times fold_by_type's count); inv_volume_sum: sum of 1 / V over the frames (replicas x samples),
    which is how per-replica boxes enter.  4 pi (r_i^2 + dr^2/12) dr is gr.jl:100-103's own shell
    volume; gr.jl normalises by N^2 / 2 pairs where N (N - 1) / 2 are counted, so for a same-slot
    row this is normalize_rdf times N / (N - 1).  Returns (r, g)."""
    row = np.asarray(row, dtype=float)
    numbins = row.shape[-1] - 1
    i = np.arange(1, numbins + 1)
    rrr = (i - 0.5) * dr
    shell = 4.0 * np.pi * (rrr * rrr + dr * dr / 12.0) * dr
    return rrr, row[..., 1:] / (float(n_site_pairs) * float(inv_volume_sum) * shell)


def normalize_rdf_solute(row, n_sites, dr, inv_volume_sum):
    """g(r) of one row of solute-water counts (Batch.rdf_solute: row[k] counts k dr < r <= (k + 1) dr):
    g(r_k) = row[k] / (n_sites inv_volume_sum 4 pi (r_k^2 + dr^2/12) dr) at r_k = (k + 1/2) dr.
    n_sites: the water sites a frame counts into the row (N for one slot; 2 N for the two hydrogen
    slots added up); inv_volume_sum: sum of 1 / V over the frames (replicas x samples).
    4 pi (r_k^2 + dr^2/12) dr is gr.jl:100-103's shell volume, which is the exact volume of the
    shell: an ideal gas gives 1 in every bin.  Returns (r, g)."""
    row = np.asarray(row, dtype=float)
    k = np.arange(row.shape[-1])
    rrr = (k + 0.5) * dr
    shell = 4.0 * np.pi * (rrr * rrr + dr * dr / 12.0) * dr
    return rrr, row / (float(n_sites) * float(inv_volume_sum) * shell)


def coordination_number(row, n_frames, dr, r_shell=None):
    """Running coordination number of one row of solute-water counts (Batch.rdf_solute): n(r) at the
    upper bin edges r = dr, 2 dr, ..., the mean number of counted water sites within r of the solute's
    point per frame.  With r_shell: the value at the last edge not beyond r_shell (the first-shell
    coordination number for r_shell = the first minimum of g) as a float; else (edges, n)."""
    row = np.asarray(row, dtype=float)
    edges = (np.arange(row.shape[-1]) + 1.0) * dr
    n = np.cumsum(row, axis=-1) / float(n_frames)
    if r_shell is None:
        return edges, n
    k = int(np.searchsorted(edges, float(r_shell) * (1.0 + 1e-12), side="right"))
    return n[..., k - 1] if k > 0 else np.zeros(row.shape[:-1])


# ---- maps around a fixed solute (include/mmc_hip.h, mmc_batch_hydration_map) -----------------------
HMAP_VEC_SCALE = 2.0 ** 30  # MMC_HMAP_VEC_SCALE: one unit of the orientation channels
HMAP_E_SCALE = 2.0 ** 20    # MMC_HMAP_E_SCALE: one unit of the energy channels, in K


def _hmap_cube(row):
    """The cells of rows [..., cells + 2] of Batch.hydration_map as [..., g, g, g] floats (the two
    tail slots dropped)."""
    row = np.asarray(row)
    cells = row.shape[-1] - 2
    g = int(round(max(cells, 0) ** (1.0 / 3.0)))
    if cells < 8 or g * g * g != cells or g % 2:
        raise ValueError("a row of Batch.hydration_map has (2 n_half)^3 + 2 entries")
    return row[..., :cells].astype(float).reshape(row.shape[:-1] + (g, g, g))


def hydration_map_centres(n_half, cell):
    """The centres of the cells of Batch.hydration_map's cube relative to the solute's reference
    point, [g, g, g, 3] with g = 2 n_half: cell (ix, iy, iz) spans (i - n_half) cell <= p <
    (i - n_half + 1) cell along each axis."""
    ax = (np.arange(-int(n_half), int(n_half)) + 0.5) * float(cell)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1)


def hydration_density(count_row, frames, n_mol, volume, cell):
    """g(x, y, z) of one count row [..., cells + 2] of Batch.hydration_map ("O", "H1" or "H2"):
    count / (frames n_mol / volume cell^3), the local density of that site over its bulk density;
    frames = replicas x samples accumulated into the row.  An ideal gas gives 1 in every cell.
    Returns [..., g, g, g]."""
    ideal = float(frames) * float(n_mol) / float(volume) * float(cell) ** 3
    return _hmap_cube(count_row) / ideal


def hydration_polarisation(vec_rows, count_O):
    """<e_z> per cell from the rows "px", "py", "pz" ([3, cells + 2]) and the "O" row of
    Batch.hydration_map: the mean unit bisector (it points from the O towards the hydrogens) of the
    waters whose O lies in the cell, [g, g, g, 3]; NaN exactly where the cell is empty.  (A water
    without a bisector is in count_O and in no orientation sum; the map's last slot counts them.)"""
    v = _hmap_cube(vec_rows)
    if v.shape[0] != 3 or v.ndim != 4:
        raise ValueError("vec_rows must be the three orientation rows [3, cells + 2]")
    n = _hmap_cube(count_O)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.moveaxis(v, 0, -1) / HMAP_VEC_SCALE / n[..., None]
    p[n == 0] = np.nan
    return p


def hydration_energy(u_rows, count_O, cell, frames):
    """The water-solute energy per cell from the rows "u_lj" and / or "u_real" ([k, cells + 2] or one
    row; several are added) and the "O" row of Batch.hydration_map.  Returns (per_water, per_volume):
    the mean u_sw in K of a water whose O lies in the cell (NaN where the cell is empty) and the
    energy density <u_sw> in K per A^3 of the cell; per_volume.sum() cell^3 is the share of <u_sw> per
    frame that the cube holds.  frames = replicas x samples accumulated into the rows."""
    u = _hmap_cube(np.atleast_2d(np.asarray(u_rows))).sum(0) / HMAP_E_SCALE
    n = _hmap_cube(count_O)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_water = u / n
    per_water[n == 0] = np.nan
    return per_water, u / (float(frames) * float(cell) ** 3)


def hydration_radial_average(row, n_half, cell, dr):
    """The average of a map over shells of cell centres: `row` [cells + 2] of Batch.hydration_map or a
    cube [g, g, g] (a density, say), shell k = the cells whose centre lies at k dr <= r < (k + 1) dr
    from the reference point, out to the inscribed sphere n_half cell.  Returns (r, mean, n_cells): the
    shell mid-points, the mean over each shell's cells (NaN for a shell without a centre; NaN cells
    are skipped) and the number of cells averaged."""
    a = np.asarray(row)
    g = 2 * int(n_half)
    cube = _hmap_cube(a) if a.ndim == 1 else a.astype(float)
    if cube.shape != (g, g, g):
        raise ValueError("row does not belong to a cube of (2 n_half)^3 cells")
    c = hydration_map_centres(n_half, cell)
    r = np.sqrt((c * c).sum(-1))
    nb = max(int(np.floor(int(n_half) * float(cell) / float(dr) * (1.0 + 1e-12))), 1)
    k = np.floor(r / float(dr)).astype(np.int64)
    ok = (k < nb) & np.isfinite(cube)
    tot = np.bincount(k[ok], weights=cube[ok], minlength=nb)
    cnt = np.bincount(k[ok], minlength=nb)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, tot / cnt, np.nan)
    return (np.arange(nb) + 0.5) * float(dr), mean, cnt


def dielectric_constant(M, temperature, volume, factor):
    """Static dielectric constant from the fluctuation of the total dipole moment under the
    conducting (tinfoil) boundary of the Ewald sum:
    eps = 1 + 4 pi factor (<M.M> - <M>.<M>) / (3 V T).  M: [samples, 3] in e A
    (mmc_batch_dipoles); temperature in K; factor: the e^2 / A -> K constant of the energies;
    volume: A^3, a scalar or one value per sample (its mean is used)."""
    M = np.asarray(M, dtype=float).reshape(-1, 3)
    mean = M.mean(0)
    fluct = (M * M).sum(1).mean() - float(mean @ mean)
    V = float(np.mean(np.asarray(volume, dtype=float)))
    return 1.0 + 4.0 * np.pi * float(factor) * fluct / (3.0 * V * float(temperature))


# ---- orientational pair correlations (include/mmc_hip.h, "Orientational pair correlations") --------
ORIENT_SCALE = 2.0 ** 30  # MMC_ORIENT_SCALE: one unit of rows 1..3 of mmc_batch_orient_corr


def _orient_hist(hist):
    h = np.asarray(hist)
    if h.ndim < 2 or h.shape[-2] != 4 or h.shape[-1] < 3:
        raise ValueError("hist must be [..., 4, numbins + 2] (mmc_batch_orient_corr)")
    return h


def kirkwood_gk(hist, n_mol, n_frames=1):
    """The distance-dependent Kirkwood factor from an mmc_batch_orient_corr histogram
    ([..., 4, numbins + 2]; sums over several calls may be added first):
    G_K(R_k) = 1 + 2 cumsum(row1[0..k]) / (2^30 N frames), k = 0..numbins + 1, R_k = k dr the outer
    edge of bin k.  n_frames: the frames summed into each histogram (calls, times the replicas for a
    summed output).  The last element takes in slot numbins + 1, every pair beyond r_max: the
    whole-box value <|sum_i u_i|^2> / N.  Returns [..., numbins + 2]."""
    h = _orient_hist(hist)
    return 1.0 + 2.0 * np.cumsum(h[..., 1, :].astype(np.float64), axis=-1) / (ORIENT_SCALE * float(n_mol) * float(n_frames))


def orient_projections(hist, n_mol, dr, inv_volume_sum):
    """(r, g, h110, h112, <P2>) at the centres of bins 1..numbins of an mmc_batch_orient_corr
    histogram ([..., 4, numbins + 2]): g(r), h110(r) = g(r) <u_i.u_j>_r and
    h112(r) = g(r) <3 (u_i.rhat)(u_j.rhat) - u_i.u_j>_r are rows 0, 1 / 2^30 and 2 / 2^30 over
    normalize_rdf_pairs' ideal-gas pair count of the shell with N (N - 1) / 2 pairs per frame
    (inv_volume_sum: the sum of 1 / V over the frames in the histogram); <P2>(r) = row3 / (2^30 row0),
    NaN where the bin is empty."""
    h = _orient_hist(hist)
    pairs = float(n_mol) * (float(n_mol) - 1.0) / 2.0
    rows = h[..., :-1].astype(np.float64)                       # bins 0..numbins
    r, g = normalize_rdf_pairs(rows[..., 0, :], pairs, dr, inv_volume_sum)
    h110 = normalize_rdf_pairs(rows[..., 1, :] / ORIENT_SCALE, pairs, dr, inv_volume_sum)[1]
    h112 = normalize_rdf_pairs(rows[..., 2, :] / ORIENT_SCALE, pairs, dr, inv_volume_sum)[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        p2 = np.where(rows[..., 0, 1:] > 0, rows[..., 3, 1:] / (ORIENT_SCALE * rows[..., 0, 1:]), np.nan)
    return r, g, h110, h112, p2


# ---- spatial distribution functions (include/mmc_hip.h, "Spatial distribution functions") ---------
def _sdf_folded(fold):
    fold = int(fold)
    if not 0 <= fold <= 3:
        raise ValueError("fold must be 0..3")
    return bool(fold & 1), bool(fold & 2)


def sdf_ideal_count(n_mol, n_frames, volume, cell, fold, site_mask):
    """What a cell of an mmc_batch_sdf grid counts in an ideal gas of the same density:
    n_frames N (N - 1) / V popcount(site_mask) cell^3 2^(folded axes).  n_frames: the frames summed
    into the grid (calls, times the replicas for a summed output); volume: A^3."""
    n_sel = bin(int(site_mask) & 7).count("1")
    if n_sel == 0:
        raise ValueError("site_mask selects no slot")
    return (float(n_frames) * float(n_mol) * (float(n_mol) - 1.0) / float(volume) * n_sel * float(cell) ** 3
            * 2.0 ** sum(_sdf_folded(fold)))


def sdf_density(grid, n_mol, n_frames, volume, cell, fold, site_mask):
    """g(x, y, z) from the counts of an mmc_batch_sdf grid ([..., g_x, g_y, g_z]; sums over several
    calls may be added first): the counts over sdf_ideal_count."""
    return np.asarray(grid).astype(np.float64) / sdf_ideal_count(n_mol, n_frames, volume, cell, fold, site_mask)


def sdf_unfold(grid, fold):
    """The full mirror-symmetric grid [..., 2 n_half, 2 n_half, 2 n_half] (float64) of a folded
    one, for plotting: along a folded axis each cell's value is shared equally between the cell and
    its mirror image, so the total is kept and the result is what fold = 0 would have counted in a
    symmetric liquid: sdf_density(sdf_unfold(grid, fold), ..., fold=0, ...) equals
    sdf_density(grid, ..., fold, ...) on both sides."""
    g = np.asarray(grid).astype(np.float64)
    if g.ndim < 3:
        raise ValueError("grid must be [..., g_x, g_y, g_z]")
    for axis, folded in zip((-3, -2), _sdf_folded(fold)):
        if folded:
            g = 0.5 * np.concatenate([np.flip(g, axis=axis), g], axis=axis)
    return g


def sdf_cell_centres(n_half, cell, fold):
    """(x, y, z): the centres of the cells along each axis of an mmc_batch_sdf grid, (k + 1/2) cell
    with k = 0 .. n_half - 1 along a folded axis and -n_half .. n_half - 1 otherwise."""
    n, c = int(n_half), float(cell)
    full, half = (np.arange(-n, n) + 0.5) * c, (np.arange(n) + 0.5) * c
    fx, fy = _sdf_folded(fold)
    return (half if fx else full), (half if fy else full), full


# ---- pair-energy distributions (include/mmc_hip.h, "Pair-energy distributions") -------------------
PAIRE_SCALE = 2.0 ** 20  # MMC_PAIRE_SCALE: one unit of rows 1 and 2 of mmc_batch_pair_energy


def pair_energy_distribution(uhist, n_mol, u_lo, u_hi, n_frames=1):
    """(centres [n_ebins], p [..., n_ebins]) from mmc_batch_pair_energy's uhist ([..., n_ebins + 2]):
    p(u), the pairs per molecule per K with pair energy in the bin, uhist[k + 1] / (N frames width);
    its integral over u is the mean number of partners in range (the two outer slots left out).
    n_frames: the frames summed into each histogram (calls, times the replicas for a summed
    output)."""
    h = np.asarray(uhist)
    if h.ndim < 1 or h.shape[-1] < 3:
        raise ValueError("uhist must be [..., n_ebins + 2] (mmc_batch_pair_energy)")
    lo, hi = float(u_lo), float(u_hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("finite u_lo < u_hi")
    n = h.shape[-1] - 2
    w = (hi - lo) / n
    centres = lo + (np.arange(n) + 0.5) * w
    return centres, h[..., 1:-1].astype(np.float64) / (float(n_mol) * float(n_frames) * w)


def pair_energy_profile(rows, n_mol, n_frames=1):
    """(<u_C>(r), <u_LJ>(r), E(R)) from mmc_batch_pair_energy's rows ([..., 3, numbins + 2]), each
    [..., numbins + 1] over bins 0..numbins: the mean Coulomb and Lennard-Jones energy (K) of a pair
    of molecules in the bin, row 1 and row 2 over 2^20 row 0 (NaN where the bin is empty; a flagged
    pair counts in row 0 only), and the cumulative pair energy per molecule
    E(R_k) = cumsum(row1 + row2)[0..k] / (2^20 N frames), R_k = k dr the outer edge of bin k: the
    potential energy per molecule that the pairs within R_k carry."""
    h = np.asarray(rows)
    if h.ndim < 2 or h.shape[-2] != 3 or h.shape[-1] < 3:
        raise ValueError("rows must be [..., 3, numbins + 2] (mmc_batch_pair_energy)")
    r = h[..., :-1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        uc = np.where(r[..., 0, :] > 0, r[..., 1, :] / (PAIRE_SCALE * r[..., 0, :]), np.nan)
        ulj = np.where(r[..., 0, :] > 0, r[..., 2, :] / (PAIRE_SCALE * r[..., 0, :]), np.nan)
    cum = np.cumsum(r[..., 1, :] + r[..., 2, :], axis=-1) / (PAIRE_SCALE * float(n_mol) * float(n_frames))
    return uc, ulj, cum


def energetic_hbonds(nhb):
    """(p [..., 9], mean [...]) from mmc_batch_pair_energy's nhb ([..., 9]): the fraction of
    molecules with k = 0..7 and 8 or more partners below u_hb, and the mean number per molecule
    (the last slot taken as 8).  NaN where no molecule was counted."""
    h = np.asarray(nhb)
    if h.ndim < 1 or h.shape[-1] != 9:
        raise ValueError("nhb must be [..., 9] (mmc_batch_pair_energy)")
    h = h.astype(np.float64)
    tot = h.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = h / tot[..., None]
        mean = (h * np.arange(9)).sum(-1) / tot
    return p, mean


# ---- partial structure factors (include/mmc_hip.h, "Partial structure factors") --------------------
SOFQ_SCALE = 2.0 ** 24  # MMC_SOFQ_SCALE: one unit of mmc_batch_structure_factor's per-replica integers


def structure_factor_shells(n_max, box):
    """(s, count, q) of the non-empty shells of mmc_batch_structure_factor: s = |n|^2 in
    1..n_max^2, count = the integer vectors n with |n|^2 = s (r_3(s)), q = 2 pi sqrt(s) / box."""
    n_max = int(n_max)
    if n_max < 1:
        raise ValueError("n_max >= 1")
    n = np.arange(-n_max, n_max + 1)
    s3 = (n * n)[:, None, None] + (n * n)[None, :, None] + (n * n)[None, None, :]
    count = np.bincount(s3[s3 <= n_max * n_max].ravel(), minlength=n_max * n_max + 1)
    count[0] = 0
    s = np.flatnonzero(count)
    return s, count[s], 2.0 * np.pi * np.sqrt(s.astype(np.float64)) / float(box)


def _sofq_rows(sq, count):
    """float64 [..., 6, shells] in units of 1 of the non-empty shells, and their counts."""
    sq, count = np.asarray(sq), np.asarray(count)
    if sq.ndim < 2 or sq.shape[-2] != 6 or count.shape != (sq.shape[-1],):
        raise ValueError("sq must be [..., 6, n_max^2 + 1] and count [n_max^2 + 1] (mmc_batch_structure_factor)")
    rows = sq / SOFQ_SCALE if np.issubdtype(sq.dtype, np.integer) else sq.astype(np.float64)
    keep = np.flatnonzero(count)
    return rows[..., keep], count[keep].astype(np.float64)


def partial_structure_factors(sq, count, n_mol, slot_types, n_frames=1):
    """Ashcroft-Langreth partial structure factors from mmc_batch_structure_factor's output:
    S_tu(q) = <rho_t rho_u*> / sqrt(N_t N_u), averaged over the shell's vectors, with rho_t the sum
    of the slot densities of type t and N_t = n_mol times the slots of that type.  sq: int64
    [..., 6, n_max^2 + 1] (per replica, units of 2^-24) or float64 (the summed output, or a sum of
    outputs over several calls); n_frames: the frames summed into it (calls, times the replicas for
    a summed output).  slot_types as fold_by_type, e.g. ("O", "H", "H"); keys are (t, u) with
    t <= u.  A cross row (a, b), a < b, enters S_tt twice (rho_a rho_b* and its conjugate) and S_tu,
    t != u, once.  Returns {(t, u): [..., shells]} over the non-empty shells, in
    structure_factor_shells' order."""
    if len(slot_types) != 3:
        raise ValueError("slot_types: three types")
    rows, cnt = _sofq_rows(sq, count)
    n_type = {t: float(n_mol) * sum(1 for u in slot_types if u == t) for t in slot_types}
    out = {}
    for k, (a, b) in enumerate(SLOT_PAIRS):
        ta, tb = slot_types[a], slot_types[b]
        key = tuple(sorted((ta, tb)))
        w = 2.0 if (a != b and ta == tb) else 1.0
        term = w * rows[..., k, :] / (np.sqrt(n_type[ta] * n_type[tb]) * cnt * float(n_frames))
        out[key] = out[key] + term if key in out else term
    return out


def charge_structure_factor(sq, count, charges, n_mol, n_frames=1):
    """S_ZZ(q) = <|sum_a q_a rho_a|^2> / N per non-empty shell from mmc_batch_structure_factor's
    output (sq and n_frames as partial_structure_factors): charges the three slot charges in e, the
    cross rows doubled.  Returns [..., shells]."""
    qa = np.asarray(charges, dtype=np.float64).ravel()
    if qa.shape != (3,):
        raise ValueError("charges: one per slot")
    rows, cnt = _sofq_rows(sq, count)
    w = np.array([(1.0 if a == b else 2.0) * qa[a] * qa[b] for a, b in SLOT_PAIRS])
    return np.tensordot(rows, w, axes=([-2], [0])) / (float(n_mol) * cnt * float(n_frames))


def dielectric_longitudinal(szz, q, n_mol, volume, temperature, factor):
    """The longitudinal dielectric response 1 - 1 / eps_L(q) = 4 pi beta factor N S_ZZ(q) / (V q^2)
    from charge_structure_factor's S_ZZ (e^2 per molecule) at q in 1 / A: volume in A^3, temperature
    in K, factor the library's e^2 / A -> K constant."""
    szz, q = np.asarray(szz, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return 4.0 * np.pi * float(factor) * float(n_mol) * szz / (float(volume) * float(temperature) * q * q)


# ---- hydrogen bonds and tetrahedral order (include/mmc_hip.h, "Local order") -----------------------
def hbonds_per_molecule(hb_hist):
    """Mean number of donated, accepted and total hydrogen bonds per molecule from an
    mmc_batch_local_order histogram ([..., 3, 9]: molecules with n = 0..8 bonds; 8 stands for 8 or
    more).  Returns [..., 3]."""
    h = np.asarray(hb_hist, dtype=float)
    if h.shape[-2:] != (3, 9):
        raise ValueError("hb_hist must be [..., 3, 9]")
    return (h * np.arange(9.0)).sum(-1) / h.sum(-1)


def tetrahedral_mean(q_sum):
    """<q> from mmc_batch_local_order's q_sum ([..., 2]: sum of the finite q_i, their number): per
    replica for [R, 2] (NaN for a replica with no finite q_i).  Average the replicas' values, or
    pass q_sum.sum(0) for the mean over all molecules."""
    s = np.asarray(q_sum, dtype=float)
    if s.shape[-1] != 2:
        raise ValueError("q_sum must be [..., 2]")
    with np.errstate(invalid="ignore", divide="ignore"):
        return s[..., 0] / s[..., 1]


def normalize_q_hist(q_hist):
    """P(q) as a density over [-3, 1] from counts [..., q_bins]: returns (q at the bin centres,
    density), the density integrating to 1 over the bins (bin width 4 / q_bins)."""
    h = np.asarray(q_hist, dtype=float)
    nb = h.shape[-1]
    dq = 4.0 / nb
    centres = -3.0 + (np.arange(nb) + 0.5) * dq
    return centres, h / (h.sum(-1, keepdims=True) * dq)


# ---- ranked neighbours, LSI, zeta, O-O-O angles (include/mmc_hip.h, "Shell order") -----------------
def _density(hist, lo, hi, what):
    """(centres, density, fraction in the last slot) of counts [..., bins + 1] over [lo, hi]."""
    h = np.asarray(hist, dtype=float)
    if h.ndim < 1 or h.shape[-1] < 2:
        raise ValueError(f"{what} must be [..., bins + 1]")
    nb = h.shape[-1] - 1
    dx = (float(hi) - float(lo)) / nb
    centres = float(lo) + (np.arange(nb) + 0.5) * dx
    inside = h[..., :nb]
    with np.errstate(invalid="ignore", divide="ignore"):
        return centres, inside / (inside.sum(-1, keepdims=True) * dx), h[..., nb] / h.sum(-1)


def neighbour_distance_distributions(rank_hist, r_list):
    """(r, p, beyond) from mmc_batch_shell_order's rank_hist ([..., n_rank, r_bins + 1]): r the bin
    centres, p[..., k - 1, :] the density of the distance to the k-th neighbour over the molecules
    that have one inside r_list (each row integrates to 1; NaN where none has), beyond[..., k - 1]
    the fraction of the molecules whose k-th neighbour is not inside r_list.  Row 5 is the d5
    distribution; the rows times (1 - beyond), summed over all ranks, are 4 pi r^2 rho g_OO(r)."""
    if np.ndim(rank_hist) < 2:
        raise ValueError("rank_hist must be [..., n_rank, r_bins + 1]")
    return _density(rank_hist, 0.0, r_list, "rank_hist")


def lsi_distribution(lsi_hist, lsi_max):
    """(I, p, undefined) from lsi_hist [..., lsi_bins + 1]: the bin centres over [0, lsi_max], the
    density of the local structure index over the molecules where it is defined (integrates to 1;
    the last bin also holds everything at or above lsi_max), and the fraction where it is not."""
    return _density(lsi_hist, 0.0, lsi_max, "lsi_hist")


def zeta_distribution(zeta_hist, lo, hi):
    """(zeta, p, undefined) from zeta_hist [..., zeta_bins + 1]: the bin centres over [lo, hi], the
    density of zeta over the molecules where it is defined (integrates to 1; the end bins also hold
    what lies outside), and the fraction where it is not."""
    return _density(zeta_hist, lo, hi, "zeta_hist")


def ooo_angle_distribution(ang_hist):
    """(theta, p, mean_cos) from ang_hist [..., ang_bins + 1], counts over equal bins of cos(theta)
    on [-1, 1] (last slot: not finite, left out): bin k covers theta from acos(c_k + dc) to
    acos(c_k) degrees, theta[k] is the middle of that span and p[..., k] the fraction of the angles
    in the bin over the span's width -- the density per degree, P(cos) sin(theta) pi / 180 averaged
    over the bin, integrating to 1 over the spans.  Both are returned in rising theta.  mean_cos
    [...] is <cos(theta)> from the bin centres."""
    h = np.asarray(ang_hist, dtype=float)
    if h.ndim < 1 or h.shape[-1] < 2:
        raise ValueError("ang_hist must be [..., ang_bins + 1]")
    nb = h.shape[-1] - 1
    edges = np.degrees(np.arccos(np.clip(-1.0 + np.arange(nb + 1) * (2.0 / nb), -1.0, 1.0)))   # falling: 180 .. 0
    cos_c = -1.0 + (np.arange(nb) + 0.5) * (2.0 / nb)
    inside = h[..., :nb]
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = inside / inside.sum(-1, keepdims=True)
        mean_cos = (frac * cos_c).sum(-1)
    theta = 0.5 * (edges[:-1] + edges[1:])
    return theta[::-1], (frac / (edges[:-1] - edges[1:]))[..., ::-1], mean_cos


def _shell_sums(sums):
    s = np.asarray(sums, dtype=float)
    if s.shape[-1] != 4:
        raise ValueError("sums must be [..., 4]")
    return s


def lsi_mean(sums):
    """<I> from mmc_batch_shell_order's sums ([..., 4]: sum of the defined I, their number, the same
    of zeta): per replica for [R, 4] (NaN where none is defined); pass sums.sum(0) for the mean over
    all molecules."""
    s = _shell_sums(sums)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s[..., 0] / s[..., 1]


def zeta_mean(sums):
    """<zeta> from mmc_batch_shell_order's sums, as lsi_mean."""
    s = _shell_sums(sums)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s[..., 2] / s[..., 3]


# ---- Voronoi cells (include/mmc_hip.h, "Voronoi cells") ---------------------------------------------
def voronoi_volume_distribution(vol_hist, v_max):
    """(V, p, beyond) from mmc_batch_voronoi's vol_hist [..., v_bins + 1]: the bin centres over
    [0, v_max), the density of the cell volume over the unflagged molecules inside it (integrates to
    1) and the fraction at or beyond v_max."""
    return _density(vol_hist, 0.0, v_max, "vol_hist")


def asphericity_distribution(eta_hist, eta_max):
    """(eta, p, beyond) from eta_hist [..., eta_bins + 1]: the bin centres over [1, eta_max), the
    density of eta = S^3 / (36 pi V^2) (1 for a sphere, 2.25 in ice Ih) and the fraction at or beyond
    eta_max."""
    return _density(eta_hist, 1.0, eta_max, "eta_hist")


def voronoi_coordination(face_hist):
    """(n, p, mean) from face_hist [..., 65]: n = 0 .. 64, p[..., n] the fraction of the unflagged
    molecules with n counted faces (geometric neighbours), mean [...] their mean number."""
    h = np.asarray(face_hist, dtype=float)
    if h.ndim < 1 or h.shape[-1] != 65:
        raise ValueError("face_hist must be [..., 65]")
    n = np.arange(65)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = h / h.sum(-1, keepdims=True)
    return n, p, (p * n).sum(-1)


def face_side_fractions(side_hist):
    """(sides, p, mean) from side_hist [..., 17]: sides = 0 .. 16, p[..., k] the fraction of the
    counted faces with k sides, mean [...] the mean number of sides (Euler: 6 - 12 / <faces>
    when every vertex joins three faces)."""
    h = np.asarray(side_hist, dtype=float)
    if h.ndim < 1 or h.shape[-1] != 17:
        raise ValueError("side_hist must be [..., 17]")
    k = np.arange(17)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = h / h.sum(-1, keepdims=True)
    return k, p, (p * k).sum(-1)


def voronoi_neighbour_gr(nbr_hist, r_list, n_summed, density):
    """(r, g) from nbr_hist [..., r_bins + 1]: the part of g_OO(r) that geometric neighbours make
    up, counts / (n_summed 4 pi r^2 dr density) at the bin centres over [0, r_list).  n_summed: the
    unflagged molecules behind the histogram (sums[..., 0], summed over what nbr_hist is summed
    over); density: molecules per volume."""
    h = np.asarray(nbr_hist, dtype=float)
    if h.ndim < 1 or h.shape[-1] < 2:
        raise ValueError("nbr_hist must be [..., r_bins + 1]")
    nb = h.shape[-1] - 1
    dr = float(r_list) / nb
    r = (np.arange(nb) + 0.5) * dr
    shell = 4.0 * np.pi * r * r * dr * float(density)
    with np.errstate(invalid="ignore", divide="ignore"):
        return r, h[..., :nb] / (np.asarray(n_summed, dtype=float)[..., None] * shell)


def _voronoi_sums(sums):
    s = np.asarray(sums, dtype=float)
    if s.shape[-1] != 8:
        raise ValueError("sums must be [..., 8]")
    return s


def voronoi_means(sums):
    """(<V>, <eta>, <faces>) from mmc_batch_voronoi's sums ([..., 8]: number summed, sum V, sum V^2,
    sum S, sum eta, sum of counted faces, sum of counted-face area, 0) over the unflagged molecules:
    per replica for [R, 8] (NaN where none); pass sums.sum(0) for the mean over all molecules."""
    s = _voronoi_sums(sums)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s[..., 1] / s[..., 0], s[..., 4] / s[..., 0], s[..., 5] / s[..., 0]


def volume_fluctuation(sums):
    """<V^2> - <V>^2 of the cell volume over the unflagged molecules, from sums as voronoi_means."""
    s = _voronoi_sums(sums)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s[..., 1] / s[..., 0]
        return s[..., 2] / s[..., 0] - mean * mean


# ---- bond order (include/mmc_hip.h, "Bond order") ---------------------------------------------------
BO_STATS = 8  # defined, undefined, flagged, truncated, solid molecules, solid clusters, largest, sum of s^2
CHILL_CLASSES = ("cubic", "hexagonal", "interfacial_ice", "clathrate", "interfacial_clathrate", "liquid")


def _bo_stats(stats):
    st = np.asarray(stats)
    if st.ndim < 1 or st.shape[-1] != BO_STATS:
        raise ValueError("stats must be [..., 8]")
    return st


def steinhardt_distribution(q_hist):
    """(q, p, undefined) from mmc_batch_bond_order's q_hist or qbar_hist ([..., q_bins + 1]): the
    bin centres over [0, 1], the density of q_l (qbar_l) over the molecules where it is defined
    (integrates to 1) and the fraction of the molecules where it is not."""
    return _density(q_hist, 0.0, 1.0, "q_hist")


def bond_correlation_distribution(c_hist):
    """(c, p, undefined) from c_hist [..., c_bins + 1]: the bin centres over [-1, 1], the density of
    c_ij over the defined directed bonds (integrates to 1) and the fraction of the bonds that are
    undefined."""
    return _density(c_hist, -1.0, 1.0, "c_hist")


def solid_fraction(stats):
    """The solid-like molecules over all molecules (defined, undefined and flagged), from stats
    [..., 8]: per replica for [R, 8]; pass stats.sum(0) for the whole batch."""
    st = _bo_stats(stats).astype(float)
    with np.errstate(invalid="ignore", divide="ignore"):
        return st[..., 4] / (st[..., 0] + st[..., 1] + st[..., 2])


def largest_nucleus(stats):
    """The size of the largest cluster of solid-like molecules, per replica, from stats [R, 8]: the
    reaction coordinate of a nucleation study (0 where nothing is solid-like)."""
    return _bo_stats(stats)[..., 6].copy()


def nucleus_size_distribution(size_hist):
    """(n_s, w_s) from size_hist ([..., N + 1], solid clusters by size): n_s the counts as floats
    and w_s = s n_s / sum s n_s, the fraction of the solid-like molecules that sit in clusters of
    size s (NaN where there are none)."""
    h = np.asarray(size_hist, dtype=float)
    if h.ndim < 1 or h.shape[-1] < 2:
        raise ValueError("size_hist must be [..., N + 1]")
    w = h * np.arange(h.shape[-1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return h, w / w.sum(-1, keepdims=True)


def chill_plus_classes(details):
    """Per-replica counts of the CHILL+ classes from a Batch.bond_order(details=True) result taken
    with the defaults (l = 3, n_nb = 4, a = staggered, b = eclipsed): int64 [R, 6] in the order of
    CHILL_CLASSES -- cubic, hexagonal, interfacial ice, clathrate, interfacial clathrate, liquid.

    This project's definition, after Nguyen and Molinero, J. Phys. Chem. B 119, 9369 (2015); compare
    with the paper before relying on a class.  With S = ab[..., 0] the staggered and E = ab[..., 1]
    the eclipsed bonds of a molecule's (up to) four, tested in this order, the first that holds:
      cubic                  S = 4
      hexagonal              S = 3 and E = 1
      clathrate              E = 4
      interfacial clathrate  E = 3
      interfacial ice        S = 2 and some neighbour (nbr) has S > 2; or S = 3 and E = 0 and some
                             neighbour has S >= 2
      liquid                 everything else, molecules with undefined q_lm included (S = E = 0)"""
    ab, nbr = np.asarray(details["ab"]), np.asarray(details["nbr"])
    if ab.ndim != 3 or ab.shape[-1] != 2 or nbr.shape[:2] != ab.shape[:2]:
        raise ValueError("details must hold ab [R, N, 2] and nbr [R, N, 16]")
    S, E = ab[..., 0].astype(np.int64), ab[..., 1].astype(np.int64)
    R = ab.shape[0]
    s_nb = np.where(nbr >= 0, np.take_along_axis(S[:, :, None], np.maximum(nbr, 0).reshape(R, -1, 1), axis=1)
                    .reshape(nbr.shape), -1)                      # S of every neighbour, -1 where none
    best = s_nb.max(-1)
    cubic = S == 4
    hexagonal = (S == 3) & (E == 1)
    clathrate = ~cubic & ~hexagonal & (E == 4)
    iclath = ~cubic & ~hexagonal & (E == 3)
    iice = ~cubic & ~hexagonal & ~clathrate & ~iclath & (((S == 2) & (best > 2)) | ((S == 3) & (E == 0) & (best >= 2)))
    liquid = ~(cubic | hexagonal | clathrate | iclath | iice)
    return np.stack([x.sum(1) for x in (cubic, hexagonal, iice, clathrate, iclath, liquid)], axis=1).astype(np.int64)


# ---- hydrogen-bond network (include/mmc_hip.h, "Hydrogen-bond network") -----------------------------
NET_STATS = 8  # bonds, sites, clusters, largest, sum of s^2, wrap mask, largest wrapping, flagged
NET_MAX_DEG = 16


def _net_stats(stats):
    st = np.asarray(stats)
    if st.ndim < 2 or st.shape[-1] != NET_STATS:
        raise ValueError("stats must be [R, ..., 8]")
    return st


def cluster_size_distribution(size_hist):
    """(n_s, w_s) from mmc_batch_hbond_network's size_hist ([..., N + 1], clusters by number of
    sites): n_s the counts as floats and w_s = s n_s / sum s n_s, the fraction of the sites that sit
    in clusters of size s (NaN where there are no sites)."""
    h = np.asarray(size_hist, dtype=float)
    if h.ndim < 1 or h.shape[-1] < 2:
        raise ValueError("size_hist must be [..., N + 1]")
    sn = h * np.arange(h.shape[-1], dtype=float)
    with np.errstate(invalid="ignore", divide="ignore"):
        return h, sn / sn.sum(-1, keepdims=True)


def percolation_probability(stats):
    """(P_any, P_all) from stats [R, ..., 8]: the fraction of the unflagged replicas in which some
    cluster wraps the box along at least one axis, and in which the wrap masks cover all three
    (NaN where every replica is flagged).  Each [...]: one value per criterion for [R, K, 8]."""
    st = _net_stats(stats)
    ok = st[..., 7] == 0
    n = ok.sum(0).astype(float)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (ok & (st[..., 5] != 0)).sum(0) / n, (ok & (st[..., 5] == 7)).sum(0) / n


def gel_fraction(stats):
    """The largest wrapping cluster over the sites, per replica and criterion, from stats
    [R, ..., 8] -> [R, ...]: 0 where nothing wraps, NaN where flagged or without sites."""
    st = _net_stats(stats)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = st[..., 6] / st[..., 1].astype(float)
    return np.where((st[..., 7] == 0) & (st[..., 1] > 0), g, np.nan)


def mean_cluster_size(size_hist, stats):
    """The mean finite-cluster size S = sum' s^2 n_s / sum' s n_s with each replica's largest
    cluster left out of both sums, from size_hist [K, N + 1] (summed over the replicas) or
    [R, K, N + 1] and stats [R, K, 8] of the same call.  Returns [K] (NaN where nothing is left)."""
    h, st = np.asarray(size_hist, dtype=np.int64), _net_stats(stats)
    if st.ndim != 3 or h.ndim not in (2, 3) or h.shape[-2] != st.shape[1] or (h.ndim == 3 and h.shape[0] != st.shape[0]):
        raise ValueError("size_hist must be [K, N + 1] or [R, K, N + 1] beside stats [R, K, 8]")
    if h.ndim == 3:
        h = h.sum(0)
    s = np.arange(h.shape[-1], dtype=np.int64)
    big = st[..., 3]
    num = (h * s * s).sum(-1) - (big * big).sum(0)
    den = (h * s).sum(-1) - big.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, num / den.astype(float), np.nan)


def bond_fractions(deg_hist):
    """f_j, the fraction of molecules with j = 0..16 bonds, from deg_hist [..., 17]."""
    h = np.asarray(deg_hist, dtype=float)
    if h.ndim < 1 or h.shape[-1] != NET_MAX_DEG + 1:
        raise ValueError("deg_hist must be [..., 17]")
    with np.errstate(invalid="ignore", divide="ignore"):
        return h / h.sum(-1, keepdims=True)


# ---- hydrogen-bond rings (include/mmc_hip.h, "Hydrogen-bond rings") ----------------------------------
RING_MAX_SIZE = 8
RING_MEMBER_BINS = 33


def _ring_hist(ring_hist):
    h = np.asarray(ring_hist, dtype=float)
    if h.ndim < 2 or h.shape[-2:] != (3, RING_MAX_SIZE + 1):
        raise ValueError("ring_hist must be [..., 3, 9]")
    return h


def ring_size_distribution(ring_hist, n_mol, n_samples=1):
    """Rings per molecule by size, [..., 9], from mmc_batch_hbond_rings' ring_hist ([..., 3, 9]; row 0,
    the rings that do not wrap the box): counts / (n_mol n_samples), n_samples the replicas (times
    frames) a summed histogram holds.  Ice Ih and Ic have 2 six-rings per molecule and nothing else."""
    h = _ring_hist(ring_hist)
    if not (n_mol > 0 and n_samples > 0):
        raise ValueError("n_mol and n_samples must be positive")
    return h[..., 0, :] / (float(n_mol) * float(n_samples))


def ring_fractions(ring_hist):
    """The fraction of the rings (row 0) that have n = 0..8 members, [..., 9]; NaN without rings."""
    h = _ring_hist(ring_hist)[..., 0, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return h / h.sum(-1, keepdims=True)


def homodromic_fraction(ring_hist):
    """By size, [..., 9]: the fraction of the rings (row 0) round which the donations run one way
    (row 2); NaN where there is no ring of that size."""
    h = _ring_hist(ring_hist)
    with np.errstate(invalid="ignore", divide="ignore"):
        return h[..., 2, :] / h[..., 0, :]


def ring_membership(member_hist):
    """The mean number of n-rings a molecule is a member of, [..., 9] (entry 0: rings of any size),
    from member_hist [..., 9, 33] (molecules by membership; the last bin, "32 or more", counts as
    32); NaN for the rows that are empty (1, 2 and those above n_max)."""
    h = np.asarray(member_hist, dtype=float)
    if h.ndim < 2 or h.shape[-2:] != (RING_MAX_SIZE + 1, RING_MEMBER_BINS):
        raise ValueError("member_hist must be [..., 9, 33]")
    with np.errstate(invalid="ignore", divide="ignore"):
        return (h * np.arange(RING_MEMBER_BINS)).sum(-1) / h.sum(-1)


# ---- Widom test-particle insertion (include/mmc_hip.h, mmc_batch_widom) ----------------------------
MMC_SLOT_WIDOM = 0x50000000  # Philox slots of an insertion: +0, +1, +2 (+3, +4, +5: pair_molecules)


def widom_mu_ex(boltz_sum, n_total, temperature):
    """mu_ex = -T ln(sum w / n) in K (energies / k_B), w = exp(-dU / T) of n insertions; the
    reference-definition value (its total energy omits the intramolecular Ewald term, see
    ewald_intra_energy)."""
    return -float(temperature) * np.log(np.asarray(boltz_sum, dtype=float) / float(n_total))


def ewald_intra_energy(offsets, charge, kappa, factor):
    """factor sum_{a<b} q_a q_b erf(kappa r_ab) / r_ab of one rigid molecule: the intramolecular
    reciprocal-space term the reference's potential() omits.  An inserted
    molecule brings it along, so the physical mu_ex is the reference-definition mu_ex minus it."""
    import math
    off = np.asarray(offsets, dtype=float).reshape(-1, 3)
    q = np.asarray(charge, dtype=float).ravel()
    e = 0.0
    for a in range(off.shape[0]):
        for b in range(a + 1, off.shape[0]):
            r = float(np.sqrt(((off[a] - off[b]) ** 2).sum()))
            e += q[a] * q[b] * math.erf(kappa * r) / r
    return factor * e


def philox_uniforms(philox, seed, ctr, slot, replica):
    """mmc_draw (csrc/mmc_propose.hpp): the two uniforms of Philox4x32-10 with key = seed and
    counter = (ctr lo, ctr hi, slot, replica); `philox(ctr4, key2) -> 4 words` is the library's
    mmc_philox4x32 (or any equal implementation)."""
    ctr = int(ctr) & (2 ** 64 - 1)
    v = philox([ctr & 0xffffffff, ctr >> 32, int(slot) & 0xffffffff, int(replica) & 0xffffffff],
               [int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff])
    a = ((int(v[0]) << 32) | int(v[1])) >> 11
    b = ((int(v[2]) << 32) | int(v[3])) >> 11
    return a * 2.0 ** -53, b * 2.0 ** -53


def shoemake_rotation(u1, u2, u3):
    """Rotation matrix of Shoemake's uniform unit quaternion (w, x, y, z) =
    (sqrt(u1) cos 2 pi u3, sqrt(1-u1) sin 2 pi u2, sqrt(1-u1) cos 2 pi u2, sqrt(u1) sin 2 pi u3),
    in k_widom_wave's arithmetic."""
    s1, s2 = np.sqrt(1.0 - u1), np.sqrt(u1)
    a, b = 2.0 * np.pi * u2, 2.0 * np.pi * u3
    w, x, y, z = s2 * np.cos(b), s1 * np.sin(a), s1 * np.cos(a), s2 * np.sin(b)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def widom_molecules(philox, seed, draw0, n_insert, replica, box, offsets):
    """Host mirror of mmc_batch_widom's generator: [n_insert][12] (atoms 0..8, COM 9..11) of the
    insertions of one replica.  Draw j uses counter draw0 + j; slots MMC_SLOT_WIDOM + 0, 1, 2 give
    u0..u5: COM = (u0, u1, u2) L, rotation shoemake_rotation(u3, u4, u5), atom a = COM + R off_a."""
    off = np.asarray(offsets, dtype=float).reshape(3, 3)
    return solute_molecules(philox, seed, draw0, n_insert, replica, box, off).reshape(int(n_insert), 12)


def solute_molecules(philox, seed, draw0, n_insert, replica, box, offsets):
    """Host mirror of mmc_batch_widom_solute's generator: [n_insert][S + 1][3] (the S sites, then
    the reference point c) of the insertions of one replica, offsets (S, 3).  The draws are
    widom_molecules': counter draw0 + j, slots MMC_SLOT_WIDOM + 0, 1, 2 give u0..u5, c = (u0, u1, u2)
    L, rotation shoemake_rotation(u3, u4, u5), site a = c + R off_a -- with water's three offsets
    the same bits as widom_molecules."""
    off = np.asarray(offsets, dtype=float).reshape(-1, 3)
    S = off.shape[0]
    out = np.empty((int(n_insert), S + 1, 3))
    for j in range(int(n_insert)):
        c = int(draw0) + j
        u0, u1 = philox_uniforms(philox, seed, c, MMC_SLOT_WIDOM, replica)
        u2, u3 = philox_uniforms(philox, seed, c, MMC_SLOT_WIDOM + 1, replica)
        u4, u5 = philox_uniforms(philox, seed, c, MMC_SLOT_WIDOM + 2, replica)
        com = np.array([u0 * box, u1 * box, u2 * box])
        R = shoemake_rotation(u3, u4, u5)
        for a in range(S):
            for d in range(3):
                out[j, a, d] = com[d] + ((R[d, 0] * off[a, 0] + R[d, 1] * off[a, 1]) + R[d, 2] * off[a, 2])
        out[j, S] = com
    return out


# ---- solute pairs (include/mmc_hip.h, "Solute pairs") ------------------------------------------------
def pair_molecules(philox, seed, draw0, n_insert, replica, box, offsets_a, offsets_b, d):
    """Host mirror of mmc_batch_widom_pair's generator for one replica: (mol_a [n_insert][S_A + 1][3],
    mol_b [n_insert][K][S_B + 1][3]), sites then the reference point.  A is solute_molecules' (slots
    MMC_SLOT_WIDOM + 0, 1, 2).  Slot +3 (u, v) gives the ray's direction n = (s cos phi, s sin phi, z),
    z = 1 - 2 u, s = sqrt(1 - z^2), phi = 2 pi v; slots +4 (u1, u2) and +5 (u3, its first uniform)
    give shoemake_rotation(u1, u2, u3) = R_B.  c_B,k = c_A + d_k n wrapped per axis (> box: - box,
    < 0: + box), site b = c_B,k + R_B off_b; n and R_B serve all K separations."""
    mol_a = solute_molecules(philox, seed, draw0, n_insert, replica, box, offsets_a)
    off = np.asarray(offsets_b, dtype=float).reshape(-1, 3)
    d = np.asarray(d, dtype=float).ravel()
    S, K = off.shape[0], d.shape[0]
    mol_b = np.empty((int(n_insert), K, S + 1, 3))
    for j in range(int(n_insert)):
        c = int(draw0) + j
        u, v = philox_uniforms(philox, seed, c, MMC_SLOT_WIDOM + 3, replica)
        u1, u2 = philox_uniforms(philox, seed, c, MMC_SLOT_WIDOM + 4, replica)
        u3, _ = philox_uniforms(philox, seed, c, MMC_SLOT_WIDOM + 5, replica)
        z = 1.0 - 2.0 * u
        s = np.sqrt(1.0 - z * z)
        phi = 2.0 * np.pi * v
        n = np.array([s * np.cos(phi), s * np.sin(phi), z])
        R = shoemake_rotation(u1, u2, u3)
        ro = np.array([[(R[e, 0] * off[b, 0] + R[e, 1] * off[b, 1]) + R[e, 2] * off[b, 2] for e in range(3)]
                       for b in range(S)])
        for k in range(K):
            cb = mol_a[j, -1] + d[k] * n
            cb = np.where(cb > box, cb - box, cb)
            cb = np.where(cb < 0, cb + box, cb)
            mol_b[j, k, :S] = cb + ro
            mol_b[j, k, S] = cb
    return mol_a, mol_b


def pair_pmf(boltz_ab, boltz_a, boltz_b, n_insert_total, temperature):
    """g_AB(d) and the potential of mean force w(d) = -T ln g_AB(d) (K) at infinite dilution from
    Batch.widom_pair's sums: boltz_ab (R, K), boltz_a (R,), boltz_b (R, K) over n_insert_total
    insertions per replica,
        g = <exp(-dU_AB / T)> / (<exp(-dU_A / T)> <exp(-dU_B / T)>).
    Returns a dict: g, w (K,) pooled over the replicas (the three averages pooled first); g_rep, w_rep
    (R, K) per replica; g_err, w_err (K,) the standard error of the per-replica values over the
    replicas (NaN for one replica)."""
    ab = np.asarray(boltz_ab, dtype=float)
    ab = ab.reshape(ab.shape[0], -1) if ab.ndim > 1 else ab.reshape(1, -1)
    R, K = ab.shape
    a = np.asarray(boltz_a, dtype=float).reshape(R)
    b = np.asarray(boltz_b, dtype=float).reshape(R, K)
    n, T = float(n_insert_total), float(temperature)
    with np.errstate(divide="ignore", invalid="ignore"):
        g_rep = (ab / n) / ((a[:, None] / n) * (b / n))
        g = (ab.sum(0) / (R * n)) / ((a.sum() / (R * n)) * (b.sum(0) / (R * n)))
        w_rep, w = -T * np.log(g_rep), -T * np.log(g)
        if R > 1:
            g_err = g_rep.std(0, ddof=1) / np.sqrt(R)
            w_err = w_rep.std(0, ddof=1) / np.sqrt(R)
        else:
            g_err = w_err = np.full(K, np.nan)
    return dict(g=g, w=w, g_rep=g_rep, w_rep=w_rep, g_err=g_err, w_err=w_err)


# ---- cavities and occupancy (include/mmc_hip.h, "Cavities and occupancy") ---------------------------
MMC_SLOT_CAVITY = MMC_SLOT_WIDOM  # the probe points are Widom's COM draws: slots +0 and +1


def cavity_points(philox, seed, draw0, n_probe, replica, box):
    """Host mirror of mmc_batch_cavity's generator: [n_probe][3], the probe points of one replica.
    Probe j uses counter draw0 + j: (u0, u1) of slot MMC_SLOT_CAVITY and the first uniform of slot
    MMC_SLOT_CAVITY + 1 give the point (u0, u1, u2) box -- widom_molecules(...)[:, 9:] bit for bit."""
    out = np.empty((int(n_probe), 3))
    for j in range(int(n_probe)):
        c = int(draw0) + j
        u0, u1 = philox_uniforms(philox, seed, c, MMC_SLOT_CAVITY, replica)
        u2, _ = philox_uniforms(philox, seed, c, MMC_SLOT_CAVITY + 1, replica)
        out[j] = (u0 * box, u1 * box, u2 * box)
    return out


def occupancy_probabilities(occ_hist, allow_overflow=False):
    """p_n per radius from mmc_batch_cavity's occ_hist ([..., K, n_cap + 1] counts): each row divided
    by its number of probes.  The last bin stands for "n_cap or more": unless allow_overflow, a count
    there is refused (p_n would be wrong at n_cap; ask for a larger n_cap).  Returns [..., K, n_cap + 1]."""
    h = np.asarray(occ_hist, dtype=np.float64)
    if h.ndim < 2:
        raise ValueError("occ_hist must be [..., K, n_cap + 1]")
    if not allow_overflow and np.any(h[..., -1] != 0):
        raise ValueError("the overflow bin (n_cap or more) is not empty: raise n_cap, or pass allow_overflow=True")
    with np.errstate(invalid="ignore", divide="ignore"):
        return h / h.sum(-1, keepdims=True)


def occupancy_moments(occ_mom, n_total):
    """(<n>, <dn^2>) per radius from mmc_batch_cavity's occ_mom ([..., K, 2]: the sums of n and n^2
    over n_total probes): the mean and the variance <n^2> - <n>^2, each [..., K]."""
    m = np.asarray(occ_mom, dtype=np.float64)
    if m.shape[-1] != 2:
        raise ValueError("occ_mom must be [..., K, 2]")
    mean = m[..., 0] / float(n_total)
    return mean, m[..., 1] / float(n_total) - mean * mean


def cavity_mu_ex(p0, temperature):
    """The excess chemical potential of a hard sphere from the probability p0 of finding its exclusion
    sphere empty: -T ln p0 in K, like widom_mu_ex (+inf where p0 is 0)."""
    with np.errstate(divide="ignore"):
        return -float(temperature) * np.log(np.asarray(p0, dtype=np.float64))


def cavity_size_distribution(nn_hist, nn_max):
    """(edges [nn_bins + 1], p0 [..., nn_bins + 1]) from mmc_batch_cavity's nn_hist ([..., nn_bins + 1]):
    edges[m] = m (nn_max / nn_bins) and p0[m] = the fraction of probes whose nearest site is at or
    beyond edges[m] -- the probability that a sphere of radius edges[m] about a random point is
    empty, on the whole grid from one pass (p0[0] = 1).  Exactly occ_hist[k][0] / probes for a radius
    that was passed as m * (nn_max / nn_bins)."""
    h = np.asarray(nn_hist)
    nb = h.shape[-1] - 1
    if nb < 1:
        raise ValueError("nn_hist must be [..., nn_bins + 1]")
    edges = np.arange(nb + 1) * (np.float64(nn_max) / nb)
    tail = np.cumsum(h[..., ::-1].astype(np.uint64), axis=-1)[..., ::-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return edges, tail.astype(np.float64) / tail[..., :1].astype(np.float64)


def information_theory_pn(mean, var, n_max, tol=1e-12, max_iter=200):
    """The two-moment information-theory model of the occupancy distribution (Hummer et al., PNAS
    93, 8951, 1996): the maximum-entropy p_n relative to a flat default model on n = 0 .. n_max with
    the given mean and variance, p_n = exp(l1 n + l2 n^2) / Z.  The two multipliers come from a
    damped Newton iteration on the convex dual ln Z - l1 <n> - l2 <n^2>, started at the continuous
    Gaussian (l2 = -1 / (2 var), l1 = mean / var).  Returns p [n_max + 1]; p[0] is the model's cavity
    probability.  Raises when the moments cannot be met on the grid."""
    mean, var, n_max = float(mean), float(var), int(n_max)
    if not (n_max >= 2 and 0.0 < mean < n_max and var > 0.0):
        raise ValueError("needs n_max >= 2, 0 < mean < n_max and var > 0")
    n = np.arange(n_max + 1, dtype=np.float64)
    f = np.stack([n, n * n])
    target = np.array([mean, var + mean * mean])
    lam = np.array([mean / var, -0.5 / var])

    def model(l):
        a = l[0] * n + l[1] * n * n
        a -= a.max()
        w = np.exp(a)
        z = w.sum()
        return w / z, np.log(z) + (l[0] * n + l[1] * n * n).max() - l @ target

    p, dual = model(lam)
    for _ in range(int(max_iter)):
        g = f @ p - target
        if np.all(np.abs(g) <= tol * np.maximum(1.0, np.abs(target))):
            return p
        d = f - (f @ p)[:, None]
        hess = (d * p) @ d.T
        try:
            step = np.linalg.solve(hess, g)
        except np.linalg.LinAlgError:
            break
        t = 1.0
        while t > 1e-10:
            p_new, dual_new = model(lam - t * step)
            if np.isfinite(dual_new) and dual_new <= dual:
                break
            t *= 0.5
        else:
            break
        lam, p, dual = lam - t * step, p_new, dual_new
    g = f @ p - target
    if np.all(np.abs(g) <= 1e-8 * np.maximum(1.0, np.abs(target))):
        return p
    raise ValueError("no two-moment distribution on 0..n_max has these moments (or the solve did not converge)")


# ---- deletion energies, overlapping distributions and BAR (include/mmc_hip.h, mmc_batch_deletion) ----
def energy_bins(du, n_bins, u_lo, u_hi):
    """mmc_batch_deletion's binning rule in numpy, for histogramming mmc_batch_widom's insertion
    energies (du_out summed to dU) on the same grid: uint64 [n_bins + 2].  With
    s = n_bins / (u_hi - u_lo) and k = floor((dU - u_lo) * s): dU < u_lo goes to slot 0, dU >= u_hi
    or k >= n_bins to slot n_bins + 1, everything else to slot k + 1.  NaN is counted nowhere
    (+-inf in the outer slots)."""
    n_bins = int(n_bins)
    lo, hi = np.float64(u_lo), np.float64(u_hi)
    if n_bins < 1 or not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("n_bins >= 1 and finite u_lo < u_hi")
    x = np.asarray(du, dtype=np.float64).ravel()
    x = x[~np.isnan(x)]
    s = np.float64(n_bins) / (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.floor((x - lo) * s)
    k = np.clip(np.where(np.isnan(k), 0.0, k), -1.0, float(n_bins)).astype(np.int64)
    slot = np.where(x < lo, 0, np.where((x >= hi) | (k >= n_bins), n_bins + 1, k + 1))
    return np.bincount(slot, minlength=n_bins + 2).astype(np.uint64)


def overlap_curves(hist_ins, hist_del, n_bins, u_lo, u_hi, temperature):
    """The overlapping-distribution (Shing-Gubbins) check from two histograms on one grid
    (energy_bins / mmc_batch_deletion, [n_bins + 2] each): f(u), the density of the insertion
    energies, and g(u), that of the deletion energies, obey g(u) = f(u) exp(-(u - mu_ex) / T), so
    ln g - ln f + u / T is the constant mu_ex / T wherever both are populated.  Each density is
    normalised by ALL of its histogram's counts, the outer slots included (add the insertions of
    weight 0 to slot n_bins + 1 before calling: they are insertions of infinite energy).  Returns
    (centres [n_bins], ln f, ln g, ln g - ln f + centres / T); an empty bin gives -inf and NaN."""
    n_bins = int(n_bins)
    hi_, hd_ = np.asarray(hist_ins, dtype=np.float64), np.asarray(hist_del, dtype=np.float64)
    if hi_.shape != (n_bins + 2,) or hd_.shape != (n_bins + 2,):
        raise ValueError("both histograms must be [n_bins + 2]")
    w = (float(u_hi) - float(u_lo)) / n_bins
    centres = float(u_lo) + (np.arange(n_bins) + 0.5) * w
    with np.errstate(divide="ignore", invalid="ignore"):
        ln_f = np.log(hi_[1:-1] / (hi_.sum() * w))
        ln_g = np.log(hd_[1:-1] / (hd_.sum() * w))
        const = np.where(np.isfinite(ln_f) & np.isfinite(ln_g), ln_g - ln_f + centres / float(temperature), np.nan)
    return centres, ln_f, ln_g, const


def bennett_mu_ex(u_ins, u_del, temperature, w_ins=None, w_del=None):
    """mu_ex (K) and its standard error by Bennett's acceptance ratio from insertion energies
    u_ins = U(N+1) - U(N) (mmc_batch_widom's du_out) and deletion energies u_del = U(N) - U(N-1)
    (mmc_batch_deletion), raw samples or bin centres with weights (counts) w_ins / w_del.  Both are
    sampled in the N-molecule system: the insertions are the forward work of N -> N+1, the
    deletions stand for the reverse work of N+1 -> N.  Identifying the N -> N-1 pair with the
    N+1 -> N pair is exact in the thermodynamic limit and costs O(1/N) in mu_ex at finite N (the
    density differs by 1/N).  Flagged (overlapping) insertions belong in u_ins with a large finite
    energy or in w_ins as counts at the top; they do not bias the estimate, dropping them does.
    Solves, by bisection on the monotone difference of the two sides,
      sum_ins fermi((u - mu) / T + M) = sum_del fermi(-(u - mu) / T - M),   M = ln(n_ins / n_del),
    fermi(x) = 1 / (1 + e^x); the variance of mu / T is Bennett's (J. Comput. Phys. 22, 245, 1976,
    in the form of Shirts et al., Phys. Rev. Lett. 91, 140601): 1 / sum_all fermi(x) fermi(-x)
    - 1 / n_ins - 1 / n_del, x = (u - mu) / T + M over both sets, for independent samples."""
    T = float(temperature)
    ui, ud = np.asarray(u_ins, dtype=np.float64).ravel(), np.asarray(u_del, dtype=np.float64).ravel()
    wi = np.ones_like(ui) if w_ins is None else np.asarray(w_ins, dtype=np.float64).ravel()
    wd = np.ones_like(ud) if w_del is None else np.asarray(w_del, dtype=np.float64).ravel()
    if wi.shape != ui.shape or wd.shape != ud.shape:
        raise ValueError("weights must match their energies")
    keep_i, keep_d = wi > 0, wd > 0
    ui, wi, ud, wd = ui[keep_i], wi[keep_i], ud[keep_d], wd[keep_d]
    if not (ui.size and ud.size and np.all(np.isfinite(ui)) and np.all(np.isfinite(ud)) and T > 0):
        raise ValueError("needs finite energies on both sides and T > 0")
    ni, nd = wi.sum(), wd.sum()
    M = np.log(ni / nd)

    def fermi(x):
        return 0.5 * (1.0 - np.tanh(0.5 * x))   # 1 / (1 + e^x) without overflow

    def diff(mu):
        return (wi * fermi((ui - mu) / T + M)).sum() - (wd * fermi(-(ud - mu) / T - M)).sum()
    pad = T * (50.0 + abs(M))
    lo, hi = min(ui.min(), ud.min()) - pad, max(ui.max(), ud.max()) + pad
    if not (diff(lo) < 0.0 < diff(hi)):
        raise ValueError("the two sets do not bracket a solution")
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if diff(mid) < 0.0:
            lo = mid
        else:
            hi = mid
    mu = 0.5 * (lo + hi)
    xi, xd = (ui - mu) / T + M, (ud - mu) / T + M
    s = (wi * fermi(xi) * fermi(-xi)).sum() + (wd * fermi(xd) * fermi(-xd)).sum()
    var = 1.0 / s - 1.0 / ni - 1.0 / nd
    return float(mu), float(T * np.sqrt(max(var, 0.0)))


# ---- virtual volume moves (include/mmc_hip.h, mmc_batch_volume_perturb) ----------------------------
def pressure_from_volume_perturbation(boltz_sum, n_calls, dv, temperature):
    """P = T ln(<w>) / dv in K / A^3 from mmc_batch_volume_perturb's sums: boltz_sum [R, K] (or [K])
    of w = (V'/V)^N exp(-dU / T) over n_calls calls, dv [K] the volume change of each test box in
    A^3 (V' - V; none zero).  Returns a dict: "per_replica" [R, K], the estimator of each replica's
    own mean; "pooled" [K], that of the mean over all replicas and calls (the estimator is the log
    of a mean, so this is not the mean of the replicas' values); and for every dv > 0 whose -dv is
    among the test boxes the two-sided average (P(+dv) + P(-dv)) / 2, whose leading error in dv
    cancels: "two_sided_dv" [P], "two_sided_per_replica" [R, P], "two_sided_pooled" [P]."""
    bs = np.atleast_2d(np.asarray(boltz_sum, dtype=float))
    dv = np.atleast_1d(np.asarray(dv, dtype=float))
    if bs.shape[1] != dv.shape[0] or np.any(dv == 0.0):
        raise ValueError("boltz_sum must be [R, K] with one non-zero dv per column")
    n, T = float(n_calls), float(temperature)
    with np.errstate(divide="ignore"):
        per = np.log(bs / n) * T / dv
        pooled = np.log(bs.sum(0) / (n * bs.shape[0])) * T / dv
    pairs = [(k, int(np.flatnonzero(dv == -dv[k])[0])) for k in range(dv.shape[0])
             if dv[k] > 0 and np.any(dv == -dv[k])]
    return {"per_replica": per, "pooled": pooled,
            "two_sided_dv": np.array([dv[k] for k, _ in pairs]),
            "two_sided_per_replica": np.stack([(per[:, k] + per[:, m]) / 2 for k, m in pairs], axis=1)
            if pairs else np.zeros((bs.shape[0], 0)),
            "two_sided_pooled": np.array([(pooled[k] + pooled[m]) / 2 for k, m in pairs])}


# ---- forces and torques (include/mmc_hip.h, mmc_batch_forces) -----------------------------------------
# hbar^2 / (k_B amu A^2) in K, from CODATA 2018: hbar = 1.054571817e-34 J s and k_B = 1.380649e-23 J/K
# (both exact by definition of the SI), amu = 1.66053906660e-27 kg, 1 A^2 = 1e-20 m^2.
HBAR_J_S = 1.054571817e-34
KB_J_PER_K = 1.380649e-23
AMU_KG = 1.66053906660e-27
HBAR2_OVER_KB_AMU_A2 = HBAR_J_S * HBAR_J_S / (KB_J_PER_K * AMU_KG * 1.0e-20)


def _fsum(fsum):
    fs = np.atleast_2d(np.asarray(fsum, dtype=np.float64))
    if fs.ndim != 2 or fs.shape[1] != 9:
        raise ValueError("fsum must be [R, 9] (or [9]): mmc_batch_forces' sums, or their sum over calls")
    return fs


def mean_square_force(fsum):
    """<F^2>, <tau^2> and <tau' I^-1 tau> per molecule from mmc_batch_forces' fsum [R, 9] (number
    summed, sum F.F, sum tau.tau, sum t, ...; sums over several calls may be added first).  Returns
    a dict: "f2", "tau2", "t" [R], each replica's own mean (NaN where nothing was summed);
    "f2_pooled", "tau2_pooled", "t_pooled", the means over all molecules of all replicas; and
    "f2_err", "tau2_err", "t_err", the standard error of the replicas' means (NaN for one replica).
    Units: (K/A)^2, K^2, K^2 / (mass unit A^2)."""
    fs = _fsum(fsum)
    n = fs[:, 0]
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name, col in (("f2", 1), ("tau2", 2), ("t", 3)):
            per = fs[:, col] / n
            out[name] = per
            out[name + "_pooled"] = float(fs[:, col].sum() / n.sum())
            ok = per[np.isfinite(per)]
            out[name + "_err"] = float(np.std(ok, ddof=1) / np.sqrt(ok.size)) if ok.size > 1 else float("nan")
    return out


def quantum_correction(fsum, temperature, mass):
    """The first-order (Wigner-Kirkwood) quantum correction to the Helmholtz free energy of a rigid
    molecule, per molecule and in K:
      dA = hbar^2 / (24 (k_B T)^2) (<F^2> / M + <tau' I^-1 tau>)
    from mmc_batch_forces' fsum [R, 9] taken WITH mass (forces in K/A, mass [3] per atom slot in
    amu, M their sum, T in K; the constant is HBAR2_OVER_KB_AMU_A2).  Returns a dict: "dA" (pooled
    over the replicas), "translational" and "rotational" (its two parts), "per_replica" [R] and
    "err", the standard error of the replicas' values."""
    T = float(temperature)
    m = np.asarray(mass, dtype=np.float64).ravel()
    if not (np.isfinite(T) and T > 0):
        raise ValueError("temperature must be positive and finite")
    if m.shape != (3,) or not (np.all(np.isfinite(m)) and np.all(m > 0)):
        raise ValueError("mass: three positive finite values (amu)")
    ms = mean_square_force(fsum)
    c = HBAR2_OVER_KB_AMU_A2 / (24.0 * T * T)
    M = (m[0] + m[1]) + m[2]
    per = c * (ms["f2"] / M + ms["t"])
    trans, rot = c * ms["f2_pooled"] / M, c * ms["t_pooled"]
    ok = per[np.isfinite(per)]
    return {"dA": float(trans + rot), "translational": float(trans), "rotational": float(rot),
            "per_replica": per,
            "err": float(np.std(ok, ddof=1) / np.sqrt(ok.size)) if ok.size > 1 else float("nan")}


# ---- the mean force, field and potential on a fixed solute (include/mmc_hip.h, mmc_batch_solute_forces) ----
def solute_mean_force(force, flags):
    """The mean over the unflagged replicas of a per-replica row of Batch.solute_forces -- force or
    torque (R, 3), or any (R, ...) -- and its standard error, the replicas being independent chains.
    Returns (mean, err, n): err is NaN for fewer than two replicas."""
    force, flags = np.asarray(force, dtype=float), np.asarray(flags)
    if flags.ndim != 1 or force.shape[:1] != flags.shape:
        raise ValueError("force (R, ...) and flags (R,) of the same replicas")
    ok = force[flags == 0]
    n = ok.shape[0]
    mean = ok.mean(axis=0) if n else np.full(force.shape[1:], np.nan)
    err = np.std(ok, axis=0, ddof=1) / np.sqrt(n) if n > 1 else np.full(force.shape[1:], np.nan)
    return mean, err, n


def pair_mean_force(site_force, mol, a, b):
    """The solvent's force along the axis of a two-body solute, per replica: (f_b - f_a) / 2 projected on
    the unit vector from site a to site b of mol (S + 1, 3) as given to Batch.set_solute (the two sites
    lie within half a box of each other).  site_force (R, S, 3) = site_lj + charge[:, None] * field of
    Batch.solute_forces(details=True).  Positive pushes the two apart."""
    sf, mol = np.asarray(site_force, dtype=float), np.asarray(mol, dtype=float)
    if a == b or sf.ndim != 3 or sf.shape[1] != mol.shape[0] - 1:
        raise ValueError("site_force (R, S, 3), mol (S + 1, 3) and two different sites")
    e = mol[b] - mol[a]
    e = e / np.sqrt(e @ e)
    return 0.5 * ((sf[:, b] - sf[:, a]) @ e)


def pmf_from_mean_force(d, f, f_err):
    """The potential of mean force W(d) = integral from d to d_max of <f>(s) ds by the cumulative
    trapezoid from the largest separation, where W = 0, with the errors of the independent points
    propagated: (W, W_err) in the order of d.  f: the mean of pair_mean_force at each separation d.
    The reference has no intramolecular term, so <f> holds the solvent's part (and the periodic images)
    alone: the caller adds the direct a-b interaction to W."""
    d, f, f_err = (np.asarray(x, dtype=float) for x in (d, f, f_err))
    if d.ndim != 1 or d.shape != f.shape or d.shape != f_err.shape or np.unique(d).size != d.size:
        raise ValueError("d, f and f_err: one value per separation, the separations all different")
    order = np.argsort(d)[::-1]                          # from the largest separation down
    x, y, s = d[order], f[order], f_err[order]
    n = x.size
    W, W_err = np.zeros(n), np.zeros(n)
    for k in range(1, n):
        wgt = np.zeros(n)                                # the trapezoid's weight of every point in W[k]
        h = x[:k] - x[1:k + 1]
        wgt[:k] += 0.5 * h
        wgt[1:k + 1] += 0.5 * h
        W[k] = (wgt * y).sum()
        W_err[k] = np.sqrt(((wgt * s) ** 2).sum())
    out, out_err = np.empty(n), np.empty(n)
    out[order], out_err[order] = W, W_err
    return out, out_err


def charging_derivative(phi, charge):
    """dU/dlambda of a solute set at charges lambda q, per replica: sum_a q_a phi_a with phi (R, S) of
    Batch.solute_forces(details=True) and the FULL charges q (S,)."""
    phi, q = np.asarray(phi, dtype=float), np.asarray(charge, dtype=float)
    if phi.ndim != 2 or phi.shape[1:] != q.shape:
        raise ValueError("phi (R, S) and charge (S,)")
    return phi @ q


def charging_free_energy(lams, mean, err):
    """The charging free energy by thermodynamic integration, the trapezoid of <sum_a q_a phi_a>_lambda
    over the coupling values lams (increasing), with the errors of the independent points propagated:
    (dA, dA_err) in K."""
    lams, mean, err = (np.asarray(x, dtype=float) for x in (lams, mean, err))
    if lams.ndim != 1 or lams.size < 2 or lams.shape != mean.shape or lams.shape != err.shape or np.any(np.diff(lams) <= 0):
        raise ValueError("lams increasing, with one mean and one error each")
    h = np.diff(lams)
    wgt = np.zeros(lams.size)
    wgt[:-1] += 0.5 * h
    wgt[1:] += 0.5 * h
    return float((wgt * mean).sum()), float(np.sqrt(((wgt * err) ** 2).sum()))


# ---- parallel tempering: per-rung views of per-replica results --------------------------------------
def by_rung(values, rung, n_rungs):
    """Regroup a per-replica array [R, ...] (energies, or the per_replica=True result of any
    observable) by the rung each replica holds: [n_rungs, n_ladders, ...], ladder l being replicas
    [l n_rungs, (l + 1) n_rungs) and `rung` (R,) what mmc_exchange_round maintains."""
    v, rung, n_rungs = np.asarray(values), np.asarray(rung), int(n_rungs)
    R = rung.shape[0]
    if rung.ndim != 1 or n_rungs < 1 or R % n_rungs or v.shape[:1] != (R,):
        raise ValueError("by_rung: rung (R,) with R a multiple of n_rungs, values [R, ...]")
    per_ladder = rung.reshape(R // n_rungs, n_rungs)
    if (np.sort(per_ladder, axis=1) != np.arange(n_rungs)).any():
        raise ValueError("by_rung: rung is not a permutation of 0..n_rungs-1 within every ladder")
    holder = np.argsort(per_ladder, axis=1) + n_rungs * np.arange(R // n_rungs)[:, None]  # [ladder, rung] -> replica
    return v[holder.T]


def exchange_acceptance(attempt, accept):
    """Acceptance ratio of every neighbouring pair of rungs (k, k + 1) from the counters of
    mmc_exchange_round; NaN where a pair was never attempted."""
    at, ac = np.asarray(attempt, dtype=np.float64), np.asarray(accept, dtype=np.float64)
    if at.shape != ac.shape:
        raise ValueError("exchange_acceptance: attempt and accept of one shape")
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(at > 0, ac / at, np.nan)


def round_trips(rung_history, n_rungs=None):
    """Completed bottom -> top -> bottom journeys of every replica from rung_history [n_rounds, R]
    (a copy of `rung` after every exchange): a journey starts when the replica is on rung 0, and
    counts when it next returns to rung 0 after having been on the top rung n_rungs - 1 (default
    max + 1 of the history).  Returns int64 (R,)."""
    h = np.asarray(rung_history)
    if h.ndim != 2:
        raise ValueError("round_trips: rung_history [n_rounds, R]")
    top = (int(h.max()) if h.size else 0) if n_rungs is None else int(n_rungs) - 1
    trips = np.zeros(h.shape[1], dtype=np.int64)
    state = np.zeros(h.shape[1], dtype=np.int8)        # 0 not started, 1 left the bottom, 2 has seen the top
    for row in h:
        trips += (state == 2) & (row == 0)
        state = np.where(row == 0, 1, np.where((row == top) & (state >= 1), 2, state)).astype(np.int8)
    return trips
