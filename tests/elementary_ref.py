"""Plain restatement of the device's own elementary functions for the tests (not a test module):
sincos_moderate of csrc/mmc_device.hpp, the argument it is given, c_mul and the power recurrence of
ewalds.jl:575-585 as the kernels apply it -- operation by operation in IEEE fp64, so that a kernel
built with -ffp-contract=off can be asked to agree BIT FOR BIT -- and exact(), the 50-digit value
of sin and cos at the fp64 argument that was actually formed.

Nothing here is derived from the device code at run time: the constants are typed in again (they are
fdlibm's, public), and fma, which Python 3.10 does not have, is the exactly rounded
a * b + c through fractions.Fraction."""
import math
from fractions import Fraction

import mpmath

TWOPI = 2.0 * 3.141592653589793   # MMC_TWOPI
FOLD_AT = 8.0e5                   # below: Cody-Waite alone; at and above: whole periods come off first
NK = 5                            # powers 1..5 of a phase factor (k_sq_max = 27)
ULP_HALF_TO_ONE = 2.0 ** -53      # one ulp of a value in [0.5, 1)
MAIN_BOUND = 2.0 ** -52           # |error| of sin and cos in the main branch (2 ulp of [0.5, 1))

_mp = mpmath.mp.clone()
_mp.dps = 50


def fma(a, b, c):
    """a * b + c with one rounding (round to nearest even), signed zeros as IEEE 754 gives them."""
    exact_sum = Fraction(a) * Fraction(b) + Fraction(c)
    if exact_sum == 0:
        prod_neg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
        if (a == 0.0 or b == 0.0) and c == 0.0:          # (+-0) + (+-0): -0 only when both are
            return -0.0 if (prod_neg and math.copysign(1.0, c) < 0) else 0.0
        return 0.0                                        # exact cancellation of non-zeros: +0
    return float(exact_sum)       # int / int true division: correctly rounded, subnormals included


def rint(x):
    """Round to the nearest integer, ties to even, the sign kept (rint(-0.3) is -0.0)."""
    return math.copysign(float(round(x)), x)


def argument(x, L):
    """The angle the kernels hand to sincos_moderate for a coordinate x in a box L:
    (MMC_TWOPI * x) / L, two roundings."""
    return (TWOPI * x) / L


def in_main_branch(arg):
    return abs(arg) < FOLD_AT


def sincos_moderate(x):
    """(sin, cos) of the angle x as csrc/mmc_device.hpp computes them."""
    if not (abs(x) < FOLD_AT):
        x = fma(-6.283185307179586, rint(x * 0.15915494309189535), x)
    fn = rint(x * 6.36619772367581382433e-01)                 # x * 2/pi
    r = fma(-fn, 1.57079632673412561417e+00, x)               # pio2_1 (33 bits)
    r = fma(-fn, 6.07710050650619224932e-11, r)               # pio2_1t
    n = int(fn)
    z = r * r
    ps = 1.58969099521155010221e-10                           # S6
    for coef in (-2.50507602534068634195e-08, 2.75573137070700676789e-06, -1.98412698298579493134e-04,
                 8.33333333332248946124e-03, -1.66666666666666324348e-01):   # S5 .. S1
        ps = fma(ps, z, coef)
    s = fma(z * r, ps, r)
    pc = -1.13596475577881948265e-11                          # C6
    for coef in (2.08757232129817482790e-09, -2.75573143513906633035e-07, 2.48015872894767294178e-05,
                 -1.38888888888741095749e-03, 4.16666666666666019037e-02):   # C5 .. C1
        pc = fma(pc, z, coef)
    c = fma(z * z, pc, fma(-0.5, z, 1.0))
    a, b = (c, s) if n & 1 else (s, c)                        # (two's complement, as in C)
    sn = -a if n & 2 else a
    cs = -b if (n + 1) & 2 else b
    return sn, cs


def phase(x, L):
    """(re, im) = (cos, sin) of argument(x, L): the phase factor e^{i 2 pi x / L} of a coordinate."""
    sn, cs = sincos_moderate(argument(x, L))
    return cs, sn


def c_mul(a, b):
    """The unfused complex product of csrc/mmc_device.hpp: (re, im)."""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def c_conj(a):
    return a[0], -a[1]


def c_rmul(q, a):
    return q * a[0], q * a[1]


ONE = (1.0, 0.0)


def powers(e1, n_max=NK):
    """[p_0 .. p_n_max]: p_0 = 1, p_1 = e1, p_k = c_mul(p_{k-1}, e1) (ewalds.jl:575-585)."""
    p = [ONE, e1]
    for _ in range(2, n_max + 1):
        p.append(c_mul(p[-1], e1))
    return p[:n_max + 1]


def signed_power(pw, k):
    """Entry k of the table k = -n_max..n_max made from powers(): negative k are conjugates."""
    return pw[k] if k >= 0 else c_conj(pw[-k])


def single_atom_S(k, px, py, pz, q=1.0):
    """S(k), k = (kx, ky, kz) with kx >= 0, of ONE atom of charge q whose phase factors are px, py,
    pz, as every RecipLong kernel forms it: ((q e^{i kx x}) e^{i ky y}) e^{i kz z} from the power
    tables, added to an accumulator that starts at +0.0 (so -0.0 never comes out); what the other
    lanes and the uncharged atoms add are zeros."""
    ex = powers(px)[k[0]]
    ey = signed_power(powers(py), k[1])
    ez = signed_power(powers(pz), k[2])
    t = c_mul(c_mul(c_rmul(q, ex), ey), ez)
    return 0.0 + t[0], 0.0 + t[1]


def kvectors(nk=NK, k_sq_max=27):
    """The reference's k-vector list in its order (ewalds.jl:57-89): kx outer, kz inner."""
    return [(kx, ky, kz) for kx in range(0, nk + 1) for ky in range(-nk, nk + 1)
            for kz in range(-nk, nk + 1) if 0 < kx * kx + ky * ky + kz * kz < k_sq_max]


def stored_axis_vectors(axis, nk=NK):
    """[(n, k)]: for n = 1..nk the member of the conjugate pair +-n along `axis` whose S(k) a batch
    computes itself -- kx > 0 for x, and of the kx = 0 plane the earlier one in the reference's
    walk, (0, -n, 0) and (0, 0, -n); the other is its conjugate, copied."""
    out = []
    for n in range(1, nk + 1):
        k = [0, 0, 0]
        k[axis] = n if axis == 0 else -n
        out.append((n, tuple(k)))
    return out


def exact(arg):
    """(sin, cos) of the fp64 number arg at 50 digits (mpmath)."""
    a = _mp.mpf(arg)
    return _mp.sin(a), _mp.cos(a)


def abs_error(value, exact_value):
    """|value - exact_value| as an mpmath number (no rounding worth the name at 50 digits)."""
    return abs(_mp.mpf(value) - exact_value)


def error_bound(arg):
    """The documented absolute accuracy of sincos_moderate at the angle arg: 2^-52 in the main
    branch; where whole periods were taken off first, the error of the period constant n times
    over stays below |arg| 2^-52, added to it."""
    if in_main_branch(arg):
        return _mp.mpf(MAIN_BOUND)
    return abs(_mp.mpf(arg)) * _mp.mpf(MAIN_BOUND) + _mp.mpf(MAIN_BOUND)


def worst_error(arg, sn, cs):
    """max(|sn - sin(arg)|, |cs - cos(arg)|) and error_bound(arg), both mpmath numbers."""
    es, ec = exact(arg)
    return max(abs_error(sn, es), abs_error(cs, ec)), error_bound(arg)


# ---- the argument families, as coordinates x in a box L ------------------------------------------
BOXES = (20.0, 30.0, 32.0)   # NIST configurations 1 (to 3) and 4; 32: exactly representable fractions


def _ulps(x, j):
    for _ in range(abs(j)):
        x = math.nextafter(x, math.inf if j > 0 else -math.inf)
    return x


def family_a(L, n, rng):
    """Coordinates within a few box lengths: uniform in [-3 L, 4 L]."""
    return [float(v) for v in rng.uniform(-3.0 * L, 4.0 * L, n)]


def family_b_targets():
    """The nearest doubles to m pi/2 and m pi/2 + pi/4, m = -40..40 (quadrant edges and the middles
    where sine and cosine change roles)."""
    out = []
    for m in range(-40, 41):
        out.append(float(_mp.mpf(m) * _mp.pi / 2))
        out.append(float(_mp.mpf(m) * _mp.pi / 2 + _mp.pi / 4))
    return out


def family_b(L, sweep=3):
    """Coordinates whose achieved argument is a family_b_targets() value or a neighbour of it.  Not
    every double is the image of a coordinate (2 pi x / L takes steps of 0.8 to 1.6 ulp), so for
    every target t the coordinates within `sweep` ulp of the one that lands closest to t are taken:
    their arguments cover t and what lies within an ulp of it on both sides, and beyond."""
    xs = []
    for t in family_b_targets():
        x0 = t * L / TWOPI
        best = min((_ulps(x0, j) for j in range(-4, 5)), key=lambda x: (abs(argument(x, L) - t), x))
        xs.extend(_ulps(best, j) for j in range(-sweep, sweep + 1))
    return xs


def family_b_fractions(L=32.0):
    """Exactly representable box fractions: 0, -0.0, +-L/4, +-L/2, +-L, 3L/4."""
    return [0.0, -0.0, L / 4, -L / 4, L / 2, -L / 2, L, -L, 3 * L / 4]


def family_c(L, n, rng):
    """Coordinates up to 1e5 box lengths away, both signs, spread over the decades from 10 L: still
    the main branch (2 pi 1e5 = 6.3e5 < 8e5)."""
    mag = L * 10.0 ** rng.uniform(1.0, 5.0, n)
    xs = [float(v) for v in mag * rng.choice([-1.0, 1.0], n)]
    return xs + [1.0e5 * L, -1.0e5 * L]


def family_d(L, n, rng):
    """The fold-back branch: achieved |argument| just below 8e5, at it, just above it, and up to
    1e9, both signs (the first entries straddle the threshold: the two branches meet there)."""
    xs = []
    x0 = FOLD_AT * L / TWOPI
    edge = min((_ulps(x0, j) for j in range(-4, 5)), key=lambda x: (abs(argument(x, L) - FOLD_AT), x))
    for j in range(-6, 7):
        xs.extend([_ulps(edge, j), -_ulps(edge, j)])
    arg = FOLD_AT * 10.0 ** rng.uniform(0.0, math.log10(1.0e9 / FOLD_AT), n)
    xs.extend(float(v) for v in arg * L / TWOPI * rng.choice([-1.0, 1.0], n))
    top = 1.0e9 * L / TWOPI
    while abs(argument(top, L)) > 1.0e9:
        top = _ulps(top, -1)
    return xs + [top, -top]


def family_e(L, n, rng):
    """Tiny coordinates: the smallest subnormal and its neighbours, the subnormal / normal border,
    and magnitudes spread over the decades up to 1e-3, both signs."""
    tiny, border = 5e-324, 2.2250738585072014e-308
    xs = [tiny, 2 * tiny, 3 * tiny, _ulps(border, -1), border, _ulps(border, 1), 1.0e-3]
    mag = 10.0 ** rng.uniform(-323.0, -3.0, n)
    xs.extend(float(v) for v in mag)
    return [s * v for v in xs for s in (1.0, -1.0)]
