"""The reference of tests/test_gpu_pivchol_regimes.py, checked on its own (no GPU): for every case of
_pivchol_reference.CASES the long-double pivoted Cholesky must find the rank and the independent columns the generator built
in, and win every pivot search by a margin that rounding in the device's double arithmetic cannot overturn - otherwise a
different pivot order on the device would be a legitimate answer and the comparison of zero rows would prove nothing.
A seed that misses a condition is replaced in CASES; the conditions stay."""
import numpy as np
import pytest

import _pivchol_reference as pr


@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_reference_finds_the_rank_and_the_independent_columns_by_a_margin(name):
    from test_gpu_fit import _pivoted_qr_basic_solution
    c = pr.case(name)
    W, r, P, Y, G = c["W"], c["r"], c["P"], c["Y"], c["G"]
    assert G.shape == (W, W) and (G == G.T).all() and c["C"].shape == (W, c["nc"])
    rel_tol = W * 64 * pr.EPS
    print("case %s: W %d rank %d margin %.2f last pivot ratio %.3g leftover %.3g (rel_tol %.3g)"
          % (name, W, len(c["order"]), c["margins"].min(), c["ratios"][-1], c["left"], rel_tol))
    assert len(c["order"]) == r == np.linalg.matrix_rank(P)
    assert np.array_equal(np.sort(c["order"]), c["ind"])
    assert c["margins"].min() >= 2.0                        # every chosen pivot against the best column that must not be chosen
    assert c["ratios"][-1] >= 1e-3
    assert c["left"] <= 1e-3 * rel_tol
    S = np.sort(c["order"])
    assert np.linalg.cond(G[np.ix_(S, S)]) <= 100
    Kq, rq = _pivoted_qr_basic_solution(P, Y)
    assert rq == r
    assert np.abs((P @ c["Kref"] - Y) - (P @ Kq - Y)).max() <= 1e-10
    assert not c["Kref"][np.setdiff1d(np.arange(W), S)].any()


@pytest.mark.parametrize("name", ["F", "I"])
def test_twins_are_bitwise_ties_and_the_lowest_index_is_the_reference_choice(name):
    """The duplicate pairs: the copy is a dependent column, the original an independent one; both orders occur; the two rows
    of G and C are equal bit for bit; the reference selects the lower index of each pair and never the higher."""
    c = pr.case(name)
    W, r, nc, seed, specs, _ = pr.CASES[name]
    ind0 = pr.make_case(W, r, nc, seed)[4]
    lower = [j < i for i, j in c["dups"]]
    assert len(c["dups"]) == len(specs) and any(lower) and not all(lower)
    assert sorted(abs(i - j) for i, j in c["dups"]) == sorted(d for d, _ in specs)
    chosen = set(c["order"].tolist())
    for i, j in c["dups"]:
        assert i in ind0 and j not in ind0
        assert (c["G"][i] == c["G"][j]).all() and (c["G"][:, i] == c["G"][:, j]).all() and (c["C"][i] == c["C"][j]).all()
        assert (c["P"][:, i] == c["P"][:, j]).all()
        assert min(i, j) in chosen and max(i, j) not in chosen
    if name == "F":
        assert any(max(p) >= 512 for p in c["dups"])                           # wave 8
        assert any(abs(i - j) == 1 and i // 64 == j // 64 for i, j in c["dups"])
    else:
        assert any(i % 1024 == j % 1024 and i != j for i, j in c["dups"])      # one thread, two of its four rows


def test_reference_stops_by_the_kernel_rule_and_breaks_ties_low():
    """The stopping rule and the tie rule on matrices small enough to do by hand."""
    order, ratios, _, left = pr.pivchol_reference(np.diag([1.0, 4.0, 4.0, 2.0, 0.0]))
    assert order.tolist() == [1, 2, 3, 0] and ratios.tolist() == [1.0, 1.0, 0.5, 0.25] and left == 0.0
    order, _, _, _ = pr.pivchol_reference(np.diag([1.0, 2.0, 4.0, -1.0]))
    assert order.tolist() == [2, 1, 0]                                           # stops at the first non-positive pivot
    order, _, _, _ = pr.pivchol_reference(np.diag([1.0, 1e-13, 1e-15]))         # rel_tol = 3 * 64 eps = 4.3e-14
    assert order.tolist() == [0, 1]
    K = pr.basic_solution(np.array([[1.0, 2.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]]), np.array([[2.0], [3.0], [5.0]]), [1, 2])
    assert np.allclose(K, [[0.0], [1.0], [3.0]])
