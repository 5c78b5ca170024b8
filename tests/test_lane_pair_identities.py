"""The IEEE identities behind the single path of the lane-pair solver (sgp_dev_solve.h, sgp_device_math.h), in numpy float32 where every operation
rounds once, as the device code does under -ffp-contract=off -fno-fast-math (no GPU, no compiler):

* v3_normalized_perpendicular: selecting the operand first (a = |n.x| > |n.y| ? n.x : n.y), then one root and two divisions, gives the bits of the two
  written-out forms, ties and special values included;
* half_apply / pos_half_solve_rec: a - b * (l * im) is a + b * ((-l) * im), and a - b * l is a + b * (-l), signed zeros included."""
import numpy as np

F = np.float32


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def perpendicular_branches(n):
    """the form with one branch per case, each with its own root and divisions (what the device code was)"""
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    out = np.zeros_like(n)
    with np.errstate(all="ignore"):
        m = np.abs(x) > np.abs(y)
        ln = np.sqrt(x[m] * x[m] + z[m] * z[m])
        out[m, 0], out[m, 1], out[m, 2] = z[m] / ln, F(0.0), -x[m] / ln
        m = ~m
        ln = np.sqrt(y[m] * y[m] + z[m] * z[m])
        out[m, 0], out[m, 1], out[m, 2] = F(0.0), z[m] / ln, -y[m] / ln
    return out


def perpendicular_select(n):
    """operand first, then ONE root and two divisions, placed by the same condition (what the device code is)"""
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        xz = np.abs(x) > np.abs(y)
        a = np.where(xz, x, y)
        ln = np.sqrt(a * a + z * z)
        u, v = z / ln, -a / ln
    zero = np.zeros_like(u)
    return np.stack([np.where(xz, u, zero), np.where(xz, zero, u), v], axis=1)


def normals():
    rng = np.random.Generator(np.random.PCG64(11))
    r = rng.standard_normal((1_000_000, 3))
    r = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F)
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    ties = []
    for a in (0.5, np.sqrt(0.5), 0.25, 1e-3):
        c = np.sqrt(max(0.0, 1.0 - 2 * a * a))
        ties += [(sx * a, sy * a, sc * c) for sx in (1, -1) for sy in (1, -1) for sc in (1, -1)]
    t = rng.standard_normal((1000, 2))
    flat = [(np.cos(p), np.sin(p), z) for p in np.linspace(0.0, 2 * np.pi, 97) for z in (0.0, -0.0)]      # n.z = 0 (both zeros)
    tiny = F(1e-40)      # denormal in float32
    assert 0 < tiny < np.finfo(F).tiny
    den = [(tiny, 1, 0), (1, tiny, 0), (0, 1, tiny), (1, 0, -tiny), (tiny, tiny, 1), (-tiny, tiny, -1), (tiny, -tiny / F(2), 1), (0.6, tiny, 0.8), (tiny, 0.6, -0.8),
           (0.0, 0.0, 1), (-0.0, 0.0, 1), (0.0, -0.0, -1)]
    rand_ties = np.stack([t[:, 0], t[:, 0] * np.sign(t[:, 1]), t[:, 1]], axis=1)
    rand_ties /= np.linalg.norm(rand_ties, axis=1, keepdims=True)
    rand_ties = rand_ties.astype(F)
    rand_ties[:, 1] = np.copysign(rand_ties[:, 0], rand_ties[:, 1])      # exact ties after rounding
    special = np.array(axes + ties + flat + den, dtype=F)
    return np.concatenate([r, special, rand_ties]), len(special) + len(rand_ties)


def test_perpendicular_with_the_operand_selected_first_has_the_bits_of_the_two_branches():
    n, n_special = normals()
    assert n.dtype == F and len(n) >= 1_000_000 + n_special
    nx, ny = np.abs(n[:, 0]), np.abs(n[:, 1])
    assert (nx > ny).sum() > 400_000 and (nx < ny).sum() > 400_000 and (nx == ny).sum() > 1000
    old, new = perpendicular_branches(n), perpendicular_select(n)
    assert old.dtype == F and new.dtype == F
    assert np.array_equal(bits(old), bits(new))
    tie = nx == ny
    assert np.all(bits(new[tie, 0]) == 0)      # a tie falls to the (0, y, z) form, with a +0 in x


def signed_values():
    rng = np.random.Generator(np.random.PCG64(12))
    n = 200_000
    v = (rng.standard_normal((4, n)) * np.exp(rng.uniform(-20, 20, (4, n)))).astype(F)
    edge = np.array([0.0, -0.0, 1.0, -1.0, 1e-40, -1e-40, 3.0e38, -3.0e38, 1e-30, -1e-30, 0.1, -0.3], dtype=F)
    grid = np.stack(np.meshgrid(edge, edge, edge, edge, indexing="ij")).reshape(4, -1)
    return np.concatenate([v, grid], axis=1)


def test_subtracting_is_adding_the_product_with_the_negated_factor():
    a, b, lam, im = signed_values()
    with np.errstate(all="ignore"):
        # linear part: lv - axis * (lambda * im)  against  lv + axis * ((-lambda) * im)
        old = a - b * (lam * im)
        new = a + b * ((-lam) * im)
        assert old.dtype == F and new.dtype == F
        same = bits(old) == bits(new)
        assert np.all(same | (np.isnan(old) & np.isnan(new)))      # (inf - inf: a NaN either way; its sign bit is not defined and never reaches a body)
        # angular part: av - iv * lambda  against  av + iv * (-lambda)
        old = a - b * lam
        new = a + b * (-lam)
        same = bits(old) == bits(new)
        assert np.all(same | (np.isnan(old) & np.isnan(new)))
        # the rotation step's argument: Ic * (-lambda) is -(Ic * lambda), which is all pos_half_solve_rec's two branches differed by
        assert np.array_equal(bits(b * (-lam)), bits(-(b * lam)))
    finite = np.isfinite(old)
    assert finite.sum() > 200_000
    zero = old == 0
    assert (zero & np.signbit(old)).any() and (zero & ~np.signbit(old)).any()      # both zeros occur among the results
