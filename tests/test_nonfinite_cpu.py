"""Non-finite state without a GPU: the case table of tests/nonfinite_cases.py does what it says in the reference's AVX
order, the list of cases on which AVX and float64 differ in class is written out, the host diagnostics agree with numpy
class for class, and the checkers that tests/test_gpu_nonfinite.py relies on reject the faults they are there to catch."""
import numpy as np
import pytest

import nbody_amd as nb
import nonfinite_cases as nc
import oracle_binding as ob
from energy_ref import energy_f64, phi_f64

DT = nc.DT
N = 700


@pytest.fixture(scope="module")
def base():
    part, m = nc.world(N, 0.6, seed=N)
    assert m == 435 and N % 64 != 0          # sources 255 and 256 exist, M - 1 is neither, the last row ends a ragged tile
    return part, m


def oracle_chain(p, m):
    one = ob.step(p, m, DT, 1)
    return one, ob.step(p, m, DT, 2)


def test_classes():
    x = np.array([0.0, -1.5, np.inf, -np.inf, np.nan, 3.4e38, 1e-45], dtype=np.float32)
    assert nc.classes(x).tolist() == [0, 0, 1, 2, 3, 0, 0]
    assert nc.classes(np.float64(np.nan)).tolist() == 3 and nc.class_counts(x) == (4, 1, 1, 1)


def expected_acc_counts(case, n, m):
    """(finite, +inf and -inf together, NaN) of the 2 n acc values after one and after two steps, in the AVX order"""
    name = case.name
    if case.kind == "contain":
        # the row itself: NaN from a NaN position, one NaN (x) from x = +inf on the first step; its velocity alone shows
        # in acc only on the second step, through the position it made
        if name.endswith("pad-seat"):
            return (2 * n, 0, 0), (2 * n, 0, 0)
        first = next(v for k, v in {"pos-nan": 2, "pos-inf-finite": 1, "vel-inf": 0, "vel-nan": 0}.items() if name.endswith(k))
        return (2 * n - first, 0, first), (2 * n - 2, 0, 2)
    if name.endswith("pos-nan") or name == "source-pos-nan":
        return (0, 0, 2 * n), (0, 0, 2 * n)
    if name.endswith("x-inf"):               # every x is dx * 0 = NaN, y stays finite but on the source's own row
        return (n - 1, 0, n + 1), (0, 0, 2 * n)
    if name.endswith("x-3e38") or name.endswith("far-1e18"):
        return (2 * n, 0, 0), (2 * n, 0, 0)
    if name.endswith("gm-inf"):              # dx * inf everywhere, 0 * inf on the source itself
        return (0, 2 * n - 2, 2), (0, 0, 2 * n)
    if name == "near-overflow":              # the six near rows; they are massless here, so the rest stays finite
        return (2 * n - 12, 12, 0), (2 * n - 12, 0, 12)
    if name == "denormal-radii":
        return (2 * (n - m), 0, 2 * m), (0, 0, 2 * n)
    if name == "zero-radius-coincidence":
        return (2 * n - 4, 0, 4), (0, 0, 2 * n)
    if name == "tiny-radius-coincidence":
        return (2 * n - 2, 0, 2), (2 * n - 2, 0, 2)
    raise AssertionError(name)


def test_the_table_is_complete(base):
    part, m = base
    names = [c.name for c in nc.cases_for(N, m)]
    assert len(names) == len(set(names)) == 9 + 20 + 4 == len(nc.CASES)


@pytest.mark.parametrize("case", nc.CASES, ids=repr)
def test_intended_classes_in_the_avx_order(base, case):
    part, m = base
    p = case.plant(part, m)
    for steps, want in zip((1, 2), expected_acc_counts(case, N, m)):
        c = nc.class_counts(ob.step(p, m, DT, steps)[:, 4:6])
        assert (c[0], c[1] + c[2], c[3]) == want, (case, steps, c)
    if case.name == "near-overflow":
        one = ob.step(p, m, DT, 1)
        c = nc.class_counts(one[:, 4:6])
        assert c[1] + c[2] >= 8 and c[1] >= 1 and c[2] >= 1 and c[0] >= N          # >= 8 +-inf, >= half the world finite
        assert np.all(np.isinf(one[N - 6:, 4:6])) and np.all(np.isfinite(one[:N - 6]))
    if case.kind == "contain":
        one = ob.step(p, m, DT, 1)
        i = case.row(N, m)
        others = np.arange(N) != i
        assert one[others].tobytes() == ob.step(nc.ordinary_tracer(p, i), m, DT, 1)[others].tobytes()


# the cases on which the reference's fp32 arithmetic and float64 differ in class, after one step or after two: fp32
# overflows G*m, the factor G*m / (r * r^2) or underflows r * r^2 where float64 does neither
AVX_F64_DIFFER = sorted([f"source-{r}-gm-inf" for r in nc.SOURCE_ROWS] +
                        ["near-overflow", "denormal-radii", "tiny-radius-coincidence"])


def test_avx_and_float64_agree_in_class_but_on_the_written_list(base):
    part, m = base
    differ = []
    for case in nc.CASES:
        p = case.plant(part, m)
        if any(not np.array_equal(nc.classes(ob.step(p, m, DT, s)[:, 0:6]), nc.classes(ob.step(p, m, DT, s, kind="f64")[:, 0:6]))
               for s in (1, 2)):
            differ.append(case.name)
    assert sorted(differ) == AVX_F64_DIFFER


@pytest.mark.parametrize("case", nc.CASES, ids=repr)
def test_the_oracle_passes_the_checker_and_the_bound_rows_are_what_they_should(base, case):
    """The rows under acc_bound are exactly "AVX-finite and float64-finite" (bound_mask takes nothing else out): >= N - 1
    of them for a containment plant.  The components where the fp32 oracle itself is out of float64's reach are pinned."""
    part, m = base
    p = case.plant(part, m)
    one, two = oracle_chain(p, m)
    min_rows = N - 1 if case.kind == "contain" else 0
    r1 = nc.assert_step_matches(one, p, m, DT, 1, min_rows=min_rows)
    r2 = nc.assert_step_matches(two, p, m, DT, 2, prev=one, min_rows=min_rows)
    for start, rows in ((p, r1), (one, r2)):
        mask, acc64, _, needed = nc.bound_mask(start, m, DT)
        _, mag = ob.acc_f64(start, m)
        avx = ob.step(start, m, DT, 1)
        want = np.isfinite(avx[:, 4:6]).all(axis=1) & np.isfinite(acc64).all(axis=1) & np.isfinite(mag).all(axis=1)
        assert np.array_equal(mask.all(axis=1), want) and rows == int(want.sum())
        lost = nc.lost_terms(start, m)
        if case.name.endswith(("x-3e38", "far-1e18", "pad-seat")):
            # the far particle's own row: every term is 0 in fp32 (r * r^2 or r^2 overflows), ~1e-23 and less in float64;
            # every other row loses the one term of a far SOURCE, far below its acc_bound
            i = case.row(N, m)
            assert np.argwhere(needed).tolist() == [[i, 0], [i, 1]] and np.all(avx[i, 4:6] == 0.0)
            assert 0.0 < np.max(np.abs(acc64[i])) < 1e-20 and np.all(np.abs(lost[i] - mag[i]) <= 1e-12 * mag[i])
            others = np.arange(N) != i
            assert np.all(lost[others] <= 1e-20 * mag[others])
        elif case.name == "near-overflow" and start is one:
            # after the 1e34 kick every distance squared overflows: all terms 0 in fp32, ~1e-15 and less in float64
            assert np.array_equal(needed, mask) and np.all(avx[:, 4:6][mask] == 0.0) and np.max(np.abs(acc64[mask])) < 1e-15
        else:
            assert not needed.any() and not lost[mask].any()          # the standing bound and nothing else


# ---- the host diagnostics against numpy ---------------------------------------------------------------------------------------

def host_diag(part):
    w = nb.World(part)
    assert np.array_equal(w.particles(), part, equal_nan=True)        # partitioned as built
    e, phi = w.energy(), w.potential()
    w.close()
    return e, phi


@pytest.mark.parametrize("m", nc.DIAG_M)
def test_host_diagnostics_agree_with_numpy_in_class(m):
    base_world, plants = nc.diag_plants(m)
    assert len(plants) == 13
    for name, row, a in [("clean", None, base_world)] + plants:
        e, phi = host_diag(a)
        with np.errstate(invalid="ignore", over="ignore"):
            want_phi = phi_f64(a, m)
            want, _ = energy_f64(a, m, want_phi)
        with np.errstate(invalid="ignore", over="ignore"):
            nc.assert_diag_matches(e, phi, want, want_phi.astype(np.float32), a, m, rel_u=1e-12, rel_phi=6e-8)
        v = nc.classes(nc.energy_vector(e)).tolist()          # kinetic potential mass px py L cx cy
        if name.endswith("vel-inf"):                          # vel.x = +inf: what the issue's numpy run gave
            assert v == [1, 0, 0, 1, 0, 1 if a[row, 1] < 0 else 2, 0, 0], (name, v)
        elif name.endswith("x-inf") and row is not None:
            assert v[6] == 1 and v[0] == 0 and v[2:5] == [0, 0, 0], (name, v)
        elif name == "massless-pos-nan":
            assert v == [0] * 8 and nc.class_counts(phi) == (m + 39, 0, 0, 1)
            e0, phi0 = host_diag(base_world)
            assert e == e0 and np.array_equal(np.delete(phi, row), np.delete(phi0, row))
        elif name == "clean":
            assert v == [0] * 8 and np.all(np.isfinite(phi))


# ---- teeth ---------------------------------------------------------------------------------------------------------------------

def test_the_step_checker_rejects_what_the_suspected_defects_look_like(base):
    part, m = base
    # an overflowing receiver: +-inf in the oracle
    p = nc.BY_NAME["near-overflow"].plant(part, m)
    one = ob.step(p, m, DT, 1)
    nc.assert_step_matches(one, p, m, DT, 1)
    bad = one.copy()
    i = N - 3
    assert np.isinf(bad[i, 4])
    bad[i, 4] = np.nan                              # the Kahan close of a +-inf block total
    bad[i, 2] = bad[i, 0] = np.nan                  # ... carried through the integrator, so only the class can tell
    with pytest.raises(AssertionError, match="classes differ"):
        nc.assert_step_matches(bad, p, m, DT, 1)
    # a NaN that leaks from a planted row into an untouched one
    c = nc.BY_NAME["contain-last-pos-nan"]
    p = c.plant(part, m)
    one = ob.step(p, m, DT, 1)
    nc.assert_step_matches(one, p, m, DT, 1, min_rows=N - 1)
    bad = one.copy()
    bad[17, 0:6] = one[N - 1, 0:6]
    assert np.isnan(bad[17, 4])
    with pytest.raises(AssertionError, match="classes differ"):
        nc.assert_step_matches(bad, p, m, DT, 1, min_rows=N - 1)
    # one finite acc moved by twice its bound, the integrator following it
    mask, ref, bound, _ = nc.bound_mask(p, m, DT)
    assert mask[40, 1] and bound[40, 1] > 0
    bad = one.copy()
    bad[40, 5] = np.float32(ref[40, 1] + 2.0 * bound[40, 1])
    bad[40, 3] = p[40, 3] + bad[40, 5] * np.float32(DT)
    bad[40, 1] = p[40, 1] + bad[40, 3] * np.float32(DT)
    with pytest.raises(AssertionError, match="outside acc_bound"):
        nc.assert_step_matches(bad, p, m, DT, 1)
    # and the rest of what it checks: the identities, the pass-through, the cap
    bad = one.copy()
    bad[5, 2] = np.nextafter(bad[5, 2], np.float32(np.inf))
    with pytest.raises(AssertionError, match="velocity"):
        nc.assert_step_matches(bad, p, m, DT, 1)
    bad = one.copy()
    bad[5, 7] = np.nextafter(bad[5, 7], np.float32(np.inf))
    with pytest.raises(AssertionError, match="mass / radius"):
        nc.assert_step_matches(bad, p, m, DT, 1)
    with pytest.raises(AssertionError, match="carry the acc bound"):
        nc.assert_step_matches(one, p, m, DT, 1, min_rows=N)


def test_the_diagnostics_checker_rejects_an_inf_turned_nan():
    m = 181
    _, plants = nc.diag_plants(m)
    name, row, a = plants[0]
    assert name == "0-vel-inf"
    e, phi = host_diag(a)
    nc.assert_diag_matches(e, phi, e, phi, a, m)
    assert e["kinetic"] == np.inf and e["momentum"][0] == np.inf
    for field, value in (("kinetic", np.nan), ("momentum", (np.nan, e["momentum"][1])), ("angular_momentum", np.nan)):
        bad = dict(e)
        bad[field] = value                          # what a dead lane's 0 * inf makes of the field
        with pytest.raises(AssertionError, match="energy fields"):
            nc.assert_diag_matches(bad, phi, e, phi, a, m)
    bad = dict(e)
    bad["momentum"] = (e["momentum"][0], e["momentum"][1] * (1 + 1e-9))
    with pytest.raises(AssertionError):
        nc.assert_diag_matches(bad, phi, e, phi, a, m)
    bad_phi = phi.copy()
    bad_phi[9] = np.nan
    with pytest.raises(AssertionError, match="Phi_i differ in class"):
        nc.assert_diag_matches(e, bad_phi, e, phi, a, m)
    bad_phi = phi.copy()
    bad_phi[9] *= np.float32(1.001)
    with pytest.raises(AssertionError, match="outside rel_phi"):
        nc.assert_diag_matches(e, bad_phi, e, phi, a, m)
