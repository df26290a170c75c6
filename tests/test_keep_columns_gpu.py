"""Kept columns (bhs_class.hip.h, "kept columns"): on the class path colIndC is a function of the rows' classes and the
classes' lists alone, so a multiply whose classes provably name the columns already in the library's own colIndC sends its
ring kernel out without the column stores (`cols_kept`); whatever may have changed the array's content or the classes makes
the next multiply write every column (`cols_refuted` where the device had to refute a launch).  Every multiply here runs on
class_path = 2 and is compared with the oracle at rel_tol = 0, columns included."""
import numpy as np
import pytest

from helpers import poisson_case
from benchmark_spgemm_using_csr_amd import facade as bhmod, gallery, _lib

pytestmark = pytest.mark.gpu
GRIDS = [(17, 16, 15), (12, 12, 12)]
_REF = {}


def _ref(oracle, key, m, A, B):
    """the oracle's product, computed once per key"""
    if key not in _REF:
        _REF[key] = oracle.spgemm(m, m, m, A[0], A[1], A[2], B[0], B[1], B[2])
    return _REF[key]


class _Case:
    """One handle on device arrays that the test may rewrite in place."""

    def __init__(self, grid, vdt=np.float64, options=(), pattern=None):
        import torch
        self.torch, self.dev, self.vdt = torch, torch.device("cuda", 0), vdt
        self.grid = grid
        self.m, self.rp, self.col, val = poisson_case("poisson27pt", *grid)
        if pattern is not None:
            self.rp, self.col = pattern(self.m, self.rp, self.col)
            val = gallery.fill_values(len(self.col))
        self.val = val.astype(vdt)
        plats = [False] * bhmod.NUM_PLATFORMS
        plats[bhmod.BHSPARSE_HIP] = True
        self.bh = bhmod.bhsparse(value_dtype=vdt)
        assert self.bh.initPlatform(plats) == 0
        assert self.bh.set_option("class_path", 2) == 0
        for k, v in options:
            assert self.bh.set_option(k, v) == 0
        self.bind(self.m, self.rp, self.col, self.val)

    def t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def bind(self, m, rp, col, val):
        self.m = m
        self.Bp, self.Bj, self.Bx = self.t(rp), self.t(col), self.t(val)
        self.Ap, self.Aj, self.Ax = self.Bp.clone(), self.Bj.clone(), self.Bx.clone()
        assert self.bh.initData_device(m, m, m, len(col), self.Ax, self.Ap, self.Aj, len(col), self.Bx, self.Bp, self.Bj) == 0

    def fetch(self):
        Cp = self.bh.get_rowptrC()
        nnzC = self.bh.get_nnzC()
        Cj = np.empty(nnzC, np.int32); Cx = np.empty(nnzC, self.vdt)
        assert self.bh.get_C(Cj, Cx) == 0
        return Cp, Cj, Cx

    def check(self, oracle, ref):
        C = self.fetch()
        res = oracle.compare(ref, C, rel_tol=0.0)
        assert res["ok"], res
        return C

    def multiply(self, oracle, ref):
        assert self.bh.spgemm() == 0
        assert "numeric_class" in {s["name"] for s in self.bh.kernel_stats()}
        return self.check(oracle, ref)

    def kept(self):
        return self.bh.get_info("cols_kept"), self.bh.get_info("cols_refuted")

    def plain_ref(self, oracle, tag="plain"):
        return _ref(oracle, (self.grid, tag), self.m, (self.rp, self.col, self.val), (self.rp, self.col, self.val))

    def close(self):
        assert self.bh.free_mem() == 0 and self.bh.freePlatform() == 0


def _three_multiplies(oracle, grid, vdt):
    """values of A and B rewritten in place between three multiplies; keep_columns 1 and 0"""
    results = {}
    for keep in (1, 0):
        c = _Case(grid, vdt, options=(("keep_columns", keep),))
        out = []
        for i in range(3):
            val = ((c.val + 2 * i) % 9 + 1).astype(vdt)           # (small integers: exact in either precision)
            c.Ax.copy_(c.t(val)); c.Bx.copy_(c.t(val)); c.torch.cuda.synchronize()
            ref = _ref(oracle, (grid, "values", i, np.dtype(vdt).name), c.m, (c.rp, c.col, val), (c.rp, c.col, val))
            out.append(c.multiply(oracle, ref))
            assert c.kept() == ((i if keep else 0), 0)
        results[keep] = out
        c.close()
    for a, b in zip(results[1], results[0]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("grid", GRIDS)
def test_three_multiplies_values_rewritten(oracle, grid):
    _three_multiplies(oracle, grid, np.float64)


@pytest.mark.parametrize("grid", GRIDS)
def test_float_build(oracle, grid):
    _three_multiplies(oracle, grid, np.float32)


@pytest.mark.parametrize("grid", GRIDS)
def test_slot_offset_between_multiplies(oracle, grid):
    """class_slot_offset moves the classifiers' home slot from one multiply to the next: the same patterns, other class
    numbers (row 0's is read back) -- the slot map names the classes by their lists and the columns are still kept."""
    c = _Case(grid, options=(("class_slot_offset", 1237),))
    ref = c.plain_ref(oracle)
    seen = []
    for i in range(3):
        c.multiply(oracle, ref)
        seen.append(c.bh.get_info("class_of_row0"))
        assert c.kept() == (i, 0)
    assert len(set(seen)) == 3 and min(seen) >= 0
    c.close()


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("grid", GRIDS)
def test_column_index_changed_under_the_live_handle(oracle, grid, which):
    """An interior row's first column moves one to the left (the row stays ascending): in A the row changes class, in B
    the rows of A that point at it do.  That multiply is the new matrix's product and keeps nothing; the next keeps again."""
    c = _Case(grid)
    ref = c.plain_ref(oracle)
    c.multiply(oracle, ref); c.multiply(oracle, ref)
    assert c.kept() == (1, 0)
    r = c.m // 2
    col2 = c.col.copy()
    assert col2[c.rp[r]] > 0
    col2[c.rp[r]] -= 1
    (c.Aj if which == "A" else c.Bj).copy_(c.t(col2)); c.torch.cuda.synchronize()
    A = (c.rp, col2 if which == "A" else c.col, c.val)
    B = (c.rp, col2 if which == "B" else c.col, c.val)
    ref2 = _ref(oracle, (grid, "moved", which), c.m, A, B)
    c.multiply(oracle, ref2)
    assert c.kept()[0] == 1
    c.multiply(oracle, ref2)
    kept, refuted = c.kept()
    assert kept == 2
    c.multiply(oracle, ref2)
    assert c.kept() == (3, refuted)
    c.close()


def test_two_data_sets_of_one_size(oracle):
    """8 x 18 x 12 after 12 x 12 x 12 on one handle: as many rows, other classes per row -- the first multiply after
    initData_device writes every column."""
    c = _Case((12, 12, 12))
    ref = c.plain_ref(oracle)
    c.multiply(oracle, ref); c.multiply(oracle, ref)
    assert c.kept() == (1, 0)
    m2, rp2, col2, val2 = poisson_case("poisson27pt", 8, 18, 12)
    assert m2 == c.m
    c.bind(m2, rp2, col2, val2)
    ref2 = _ref(oracle, ((8, 18, 12), "plain"), m2, (rp2, col2, val2), (rp2, col2, val2))
    c.multiply(oracle, ref2)
    assert c.kept() == (1, 0)
    c.multiply(oracle, ref2)
    assert c.kept() == (2, 0)
    c.close()


@pytest.mark.parametrize("grid", GRIDS)
def test_external_arrays_then_the_pool(oracle, grid):
    """A multiply into bound arrays leaves the pool's as they were: after unbinding, the pool's columns are complete."""
    c = _Case(grid)
    ref = c.plain_ref(oracle)
    c.multiply(oracle, ref); c.multiply(oracle, ref)
    assert c.kept() == (1, 0)
    nnzC = c.bh.get_nnzC()
    extJ = c.torch.full((nnzC,), -7, dtype=c.torch.int32, device=c.dev)
    extX = c.torch.zeros(nnzC, dtype=c.torch.float64, device=c.dev)
    assert c.bh.set_output_device(extJ, extX, nnzC) == 0
    assert c.bh.spgemm() == 0
    c.torch.cuda.synchronize()
    assert oracle.compare(ref, (c.bh.get_rowptrC(), extJ.cpu().numpy(), extX.cpu().numpy()), rel_tol=0.0)["ok"]
    assert c.kept() == (1, 0)
    assert c.bh.set_output_device(None, None, 0) == 0
    c.multiply(oracle, ref)                               # (writes: the state was dropped with the binding)
    assert c.kept() == (1, 0)
    c.multiply(oracle, ref)
    assert c.kept() == (2, 0)
    c.close()


@pytest.mark.parametrize("grid", GRIDS)
def test_other_writers_of_C_in_between(oracle, grid):
    """Between keeping multiplies: the semiring multiply, an in-place add, a selection, a masked call, a general-pipeline
    multiply.  The columns after the next ordinary multiply are the oracle's each time."""
    c = _Case(grid)
    ref = c.plain_ref(oracle)
    c.multiply(oracle, ref); c.multiply(oracle, ref)
    assert c.kept() == (1, 0)
    m = c.m
    eye_p = np.arange(m + 1, dtype=np.int32); eye_j = np.arange(m, dtype=np.int32); eye_x = np.ones(m)

    def semiring():
        assert c.bh.spgemm_semiring(_lib.BHS_SR_MIN_PLUS) == 0

    def add_in_place():
        assert c.bh.spgemm_add(1.0, 2.0, eye_p, eye_j, eye_x) == 0
        assert c.bh.get_info("add_inplace_used") == 1

    def select():
        assert c.bh.spgemm_select(bhmod.select_spec(band=(-3, 3))) == 0

    def masked():
        c.bh.spgemm_masked(c.rp, c.col)

    def general():
        assert c.bh.set_option("class_path", 0) == 0
        assert c.bh.spgemm() == 0
        c.check(oracle, ref)
        assert c.bh.set_option("class_path", 2) == 0

    for other in (semiring, add_in_place, select, masked, general):
        other()
        c.multiply(oracle, ref)
        c.multiply(oracle, ref)
    assert c.kept()[1] == 0 and c.kept()[0] >= 1 + 5
    c.close()


@pytest.mark.parametrize("grid", GRIDS)
def test_mixed_mode_stays_out(oracle, grid):
    """One perturbed row (300 consecutive entries: a row without a class): the multiplies run the mixed flow and keep nothing."""
    c = _Case(grid, pattern=lambda m, rp, col: gallery.perturb_rows_csr(rp, col, m, 0.0, long_row=(m // 2 + 7, 300)))
    ref = c.plain_ref(oracle, "one_long_row")
    for _ in range(3):
        c.multiply(oracle, ref)
        assert c.kept() == (0, 0)
    c.close()
