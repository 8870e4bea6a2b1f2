"""gram.halo_plan without a GPU: the batches of a walk that carries a halo of bins from one batch to the next tile the
bins in order, never hold an empty batch, keep every scratch of rows * (bins + halo in front) bytes inside the budget --
down to one bin a batch where the budget does not exceed the halo -- and give the walker the halo min(halo, first bin)."""
import pytest

from muahuff import gram

ROWS = 12


def _budgets(n, halo):
    """from below rows * halo to above rows * n, with the edges on either side of both"""
    marks = {1, ROWS - 1, ROWS, ROWS + 1, ROWS * halo - 1, ROWS * halo, ROWS * halo + 1, ROWS * (halo + 1), ROWS * (halo + 1) + 5,
             ROWS * (halo + 8), ROWS * (2 * halo + 3), ROWS * (n // 3 + halo) + 7, ROWS * n - 1, ROWS * n, ROWS * (n + halo), ROWS * (n + halo) + 100}
    return sorted(b for b in marks if b >= 1)


@pytest.mark.parametrize("halo", [0, 1, 14, 213])
@pytest.mark.parametrize("n", [0, 1, 7, 1000])
def test_the_batches_tile_the_bins_inside_the_budget(n, halo):
    for budget in _budgets(n, halo):
        plan = gram.halo_plan(n, ROWS, halo, budget)
        if n == 0:
            assert plan == []
            continue
        at = 0
        for b0, nb in plan:
            assert b0 == at and nb >= 1, (budget, plan[:4])
            h = min(halo, b0)                                       # what gram.walk keeps in front of the batch
            cap = budget // ROWS
            if cap > h:
                assert ROWS * (nb + h) <= budget, (budget, b0, nb)
                assert nb == min(cap - h, n - b0)                   # and no smaller than it has to be
            else:
                assert nb == 1, (budget, b0, nb)
            at += nb
        assert at == n


def test_the_halo_of_the_walk_is_the_bins_read_so_far_up_to_the_halo():
    plan = gram.halo_plan(1000, ROWS, 14, ROWS * 8)                  # fewer bins a batch than the halo
    assert plan[0] == (0, 8) and plan[1] == (8, 1) and len(plan) > 900
    assert [min(14, b0) for b0, _nb in plan[:4]] == [0, 8, 9, 10]
    plan = gram.halo_plan(1000, ROWS, 14, ROWS * 114)
    assert plan[:3] == [(0, 114), (114, 100), (214, 100)] and plan[-1] == (914, 86)
    assert gram.halo_plan(1000, ROWS, 0, ROWS * 300) == gram.batches(1000, ROWS, ROWS * 300)
    with pytest.raises(ValueError):
        gram.halo_plan(10, ROWS, -1, 100)
