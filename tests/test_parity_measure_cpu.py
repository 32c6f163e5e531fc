"""No GPU: the arithmetic that the per-entry float64 sweeps share (tests/parity_measure.py) on hand-made arrays, and what each
sweep's own `measure` decides by itself: how a NaN or an infinity of the reference has to be met, with check=True (an
AssertionError) and check=False (inf), and the matching case that it accepts.

The numbers are chosen so that nothing rounds: with s = 2^20 the derived term SUM_DEPTH u s is exactly 1.0.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_parity as AP                        # noqa: E402
import convnext_parity as CP                    # noqa: E402
import loss_parity as LP                        # noqa: E402
import parity_measure as PM                     # noqa: E402
import query_selection_ref as QR                # noqa: E402
import reid_parity as RP                        # noqa: E402
import test_query_selection_parity_gpu as QP    # noqa: E402
import tracker_parity as TP                     # noqa: E402

S = 2.0 ** 20           # SUM_DEPTH * U * S == 1.0
NAN, INF = float("nan"), float("inf")
A = lambda *v: np.array(v, dtype=np.float64)
UP = np.nextafter(1.0, 2.0)


@pytest.fixture(autouse=True)
def tables_left_as_found():
    """What these tests add to a sweep's TABLE and WORST is taken out again: the sweeps' own tests report from them."""
    mods = (AP, CP, LP, QP, RP, TP)
    saved = [(len(m.TABLE), dict(getattr(m, "WORST", {}))) for m in mods]
    yield
    for m, (n, worst) in zip(mods, saved):
        del m.TABLE[n:]
        if hasattr(m, "WORST"):
            m.WORST.clear()
            m.WORST.update(worst)


# ------------------------------------------------------------------------------------------------------- the shared arithmetic

def test_the_constants_live_here_and_are_what_they_were():
    assert (PM.U, PM.SUM_DEPTH, PM.COMP_MARGIN) == (2.0 ** -24, 16.0, 8.0) and PM.SUM_DEPTH * PM.U * S == 1.0
    for mod in (QR, AP, CP, LP, RP, TP):
        assert mod.entry_bound is PM.entry_bound and (mod.U, mod.SUM_DEPTH, mod.COMP_MARGIN) == (PM.U, PM.SUM_DEPTH, PM.COMP_MARGIN)
    assert PM.entry_bound(A(0.0, 0.5, 0.125), A(S, S, S)).tolist() == [1.0, 4.0, 1.0]


def test_an_entry_at_its_bound_passes_and_one_step_above_fails_and_is_named():
    e = PM.errors(A(1.0, 4.0), A(0.0, 0.0), A(S, S), A(0.0, 0.5))
    assert e.bound.tolist() == [1.0, 4.0] and e.ratio.tolist() == [1.0, 1.0] and e.worst == 1.0
    e.check("at the bound")
    e = PM.errors(A(0.5, UP, 0.25), A(0.0, 0.0, 0.0), A(S, S, S), A(0.0, 0.0, 0.0))
    assert e.worst == UP and e.at == (1,)
    with pytest.raises(AssertionError) as x:
        e.check("case", "output")
    assert x.value.args[0][:3] == ("case", "output", "entries over their bound") and [1] in x.value.args[0][4]


def test_bound_zero():
    e = PM.errors(A(2.0, 2.0, 3.0), A(2.0, 2.5, 3.0), A(0.0, 0.0, S), A(2.0, 2.5, 3.0))
    assert e.bound.tolist() == [0.0, 0.0, 1.0] and e.ratio.tolist() == [0.0, INF, 0.0] and e.worst == INF
    with pytest.raises(AssertionError):
        e.check()
    assert PM.quotient(A(0.0, 1.0, 1.0), A(0.0, 0.0, 4.0)).tolist() == [0.0, INF, 0.25]


def test_an_empty_input_gives_zero():
    z = np.zeros((0, 4))
    e = PM.errors(z, z, z, z)
    assert e.worst == 0.0 and isinstance(e.worst, float)
    e.check()


def test_a_nan_error_fails_the_bound_assertion():
    e = PM.Errors(A(0.0, NAN), A(0.0, 0.0), A(1.0, 1.0), A(S, S))
    assert not (e.err > e.bound).any()                  # the other way of writing it lets the NaN through
    with pytest.raises(AssertionError):
        e.check()


def test_a_non_finite_composition_term_leaves_the_derived_term_standing():
    e = PM.errors(A(1.0, 1.0, UP), A(0.0, 0.0, 0.0), A(S, S, S), A(INF, NAN, -INF))
    assert e.cerr.tolist() == [0.0, 0.0, 0.0] and e.bound.tolist() == [1.0, 1.0, 1.0] and e.ratio.tolist() == [1.0, 1.0, UP]


def test_the_row_is_relative_to_the_entrys_own_magnitude():
    e = PM.errors(A(4.5, 0.25), A(4.0, 0.0), A(S, S), A(4.25, 0.0))
    assert e.cerr.tolist() == [0.25, 0.0] and e.bound.tolist() == [2.0, 1.0] and e.at == (0,)
    assert e.row() == (0.125, 0.0625, 0.5, 0.25)
    e = PM.errors(A(4.0, 0.5), A(4.0, 0.0), A(S, S), A(4.0, 0.0))          # the worst entry's reference is 0: unit 1
    assert e.row() == (0.5, 0.0, 1.0, 0.5)


def test_the_inputs_helpers():
    assert PM.rng("a").randint(0, 1 << 30) == PM.rng("a").randint(0, 1 << 30) != PM.rng("b").randint(0, 1 << 30)
    for mod in (TP, RP, LP):
        assert (mod._rng, mod.dy, mod.is_dyadic) == (PM.rng, PM.dy, PM.is_dyadic)
    d = PM.dy(A(0.3, -0.0001, 3.0))
    assert d.dtype == np.float32 and d.tolist() == [307 / 1024.0, 0.0, 3.0] and not np.signbit(d[1])
    assert PM.dy(A(0.3), 2.0).tolist() == [614 / 1024.0] and PM.dy(A(0.3), step=64.0).tolist() == [19 / 64.0]
    assert PM.is_dyadic(d) and not PM.is_dyadic(A(0.3)) and not PM.is_dyadic(A(NAN)) and not PM.is_dyadic(A(2.0 ** 13))
    assert PM.is_dyadic(A(1 / 64.0), 64.0) and not PM.is_dyadic(A(1 / 128.0), 64.0) and not PM.is_dyadic(A(64.0), 64.0, 64.0)


def test_the_table(tmp_path, monkeypatch, capsys):
    t = PM.Table("head", env="PARITY_MEASURE_TEST_TABLE")
    t.add("a", "k", 0.5)
    t.add("b", "k", 0.25)
    t.add("c", "k", 0.75)
    t.add("dash")
    assert t.lines == ["a", "b", "c", "dash"] and t.worst == {"k": (0.75, "c")}
    monkeypatch.delenv("PARITY_MEASURE_TEST_TABLE", raising=False)
    t.report(1)
    assert capsys.readouterr().out == "head\nb\nc\ndash\n"
    path = tmp_path / "table.txt"
    monkeypatch.setenv("PARITY_MEASURE_TEST_TABLE", str(path))
    t.report(2)
    t.report(0)
    assert path.read_text() == "c\ndash\na\nb\nc\ndash\n"
    path.unlink()
    PM.Table("head").report(0)                                              # no variable: prints only
    assert capsys.readouterr().out.endswith("head\n\n") and not path.exists()


# ---------------------------------------------------------------------------------------------------- each sweep's own policy

E = 2.0 ** -16          # an error well under every sweep's tolerance (1e-4 of a scale of at least 1) ...
SE = S * 2 * E          # ... and the s whose derived term is 2 E: an entry off by E measures 0.5
HUGE = 2.0 ** 40        # an s under which only the project's tolerance is left to object


def refused(measure, *args, **kw):
    """What the sweep does not accept: check=True raises, check=False (where there is one) returns inf; no line either way."""
    table = sys.modules[measure.__module__].TABLE
    n = len(table)
    with pytest.raises(AssertionError):
        measure(*args, **kw)
    if measure is not QP.measure:
        assert measure(*args, check=False, **kw) == INF
    assert len(table) == n


def over_the_tolerance(measure, *args, **kw):
    """Inside its entry's bound and over the project's tolerance: an AssertionError that names it."""
    with pytest.raises(AssertionError) as x:
        measure(*args, **kw)
    assert "the project's bound" in x.value.args[0]


def test_query_selection_infinities_are_identical_and_in_place():
    want, mag, comp = A([1.0, INF], [-INF, 2.0]), A([SE, 0.0], [0.0, SE]), A([1.0, INF], [INF, 2.0])
    got = lambda *v: torch.tensor(v, dtype=torch.float32).view(2, 2)
    n = len(QP.TABLE)
    assert QP.measure("c", "o", got(1.0, INF, -INF, 2.0 + E), want, mag, comp) == 0.5
    assert QP.measure("c", "o", got(1.0, INF, -INF, 2.0 + E), want, mag, comp, per_row=True) == 0.5
    assert len(QP.TABLE) == n + 2 and QP.TABLE[n] == "%-30s %-16s %10.2e %10.2e %10.2e %7.3f" % ("c", "o", E / 2, 0.0, E, 0.5)
    refused(QP.measure, "c", "o", got(1.0, INF, INF, 2.0), want, mag, comp)             # the other infinity
    refused(QP.measure, "c", "o", got(1.0, 3e38, -INF, 2.0), want, mag, comp)           # a large number is no infinity
    refused(QP.measure, "c", "o", got(INF, INF, -INF, 2.0), want, mag, comp)            # one too many
    refused(QP.measure, "c", "o", got(NAN, INF, -INF, 2.0), want, mag, comp)            # no NaN
    refused(QP.measure, "c", "o", got(1.0, INF, -INF, 2.0), want, mag, A([1.0, INF], [3.0, 2.0]))     # the composition's places
    over_the_tolerance(QP.measure, "c", "o", got(1.0, INF, -INF, 2.0 + 4 * QP.C.TOL), want, A([SE, 0.0], [0.0, HUGE]), comp)   # TOL * max|want|
    inf = A(INF, INF)
    assert QP.measure("c", "o", torch.tensor([INF, INF]), inf, A(0.0, 0.0), inf) == 0.0 and "-" in QP.TABLE[-1].split()


def test_attention_nan_is_a_whole_row_and_the_same_row():
    want, mag = A([1.0, 2.0], [NAN, NAN]), A([SE, SE], [NAN, NAN])
    n = len(AP.TABLE)
    assert AP.measure("dec/x", "out", A([1.0 + E, 2.0], [NAN, NAN]), want, mag, want) == 0.5
    assert len(AP.TABLE) == n + 1 and AP.WORST[("dec", "out")] == (0.5, AP.TABLE[n])
    refused(AP.measure, "dec/x", "out", A([1.0, 2.0], [0.0, 0.0]), want, mag, want)     # a number where the row is NaN
    refused(AP.measure, "dec/x", "out", A([NAN, 2.0], [NAN, NAN]), want, mag, want)     # a NaN where it is not
    over_the_tolerance(AP.measure, "dec/x", "out", A([1.0, 2.0 + 4 * AP.TOL], [NAN, NAN]), want, A([SE, HUGE], [NAN, NAN]), want)   # TOL * max|want|
    half = A([1.0, 2.0], [3.0, NAN])
    with pytest.raises(AssertionError):                                                 # half a row: the reference itself
        AP.measure("dec/x", "out", half, half, mag, half, check=False)
    with pytest.raises(AssertionError):                                                 # the composition's rows
        AP.measure("dec/x", "out", want, want, mag, A([1.0, 2.0], [3.0, 4.0]), check=False)
    nan, n = A([NAN, NAN]), len(AP.TABLE)
    assert AP.measure("dec/x", "out", nan, nan, nan, nan) == 0.0 and "-" in AP.TABLE[-1].split() and len(AP.TABLE) == n + 1


def test_convnext_knows_no_nan():
    case = next(iter(CP.CASES))
    want, mag = A(1.0, 2.0, 0.0), A(SE, SE, SE)
    n = len(CP.TABLE)
    assert CP.measure(case, A(1.0, 2.0 + E, 0.0), want, mag, want) == 0.5 and len(CP.TABLE) == n + 1
    assert CP.WORST[(CP.CASES[case]["kernel"], CP.CASES[case]["stress"])][1] == CP.TABLE[n]
    refused(CP.measure, case, A(1.0, NAN, 0.0), want, mag, want)
    over_the_tolerance(CP.measure, case, A(1.0, 2.0 + 4 * CP.TOL, 0.0), want, A(SE, HUGE, SE), want)       # tol(want) = TOL * 2
    for bad in (dict(want=A(1.0, NAN, 0.0), comp=want), dict(want=want, comp=A(1.0, NAN, 0.0))):
        with pytest.raises(AssertionError):
            CP.measure(case, want, bad["want"], mag, bad["comp"], check=False)


def test_tracker_skips_where_the_reference_is_nan():
    want, mag, comp = A(1.0, NAN, 2.0), A(SE, NAN, SE), A(1.0, NAN, 2.0)
    n = len(TP.TABLE)
    assert TP.measure("c", "memo", "plain", A(1.0, 123.0, 2.0 + E), want, mag, comp) == 0.5     # anything may stand there
    assert TP.measure("c", "memo", "plain", A(1.0, NAN, 2.0 + E), want, mag, comp) == 0.5
    assert len(TP.TABLE) == n + 2 and TP.WORST[("memo", "plain")] == (0.5, TP.TABLE[n])
    refused(TP.measure, "c", "memo", "plain", A(NAN, NAN, 2.0), want, mag, comp)
    over_the_tolerance(TP.measure, "c", "memo", "plain", A(0.5, 0.0, 0.25 + 2 * TP.TOL), A(0.5, NAN, 0.25), A(SE, NAN, HUGE), A(0.5, NAN, 0.25))   # TOL * max(1, .)
    with pytest.raises(AssertionError):
        TP.measure("c", "memo", "plain", want, want, mag, A(NAN, NAN, 2.0), check=False)
    n = len(TP.TABLE)
    assert TP.measure("c", "memo", "plain", A(1.0), A(NAN), A(NAN), A(NAN)) == 0.0 and len(TP.TABLE) == n


def test_reid_meets_a_nan_or_an_infinity_as_such():
    want, mag, comp = A(-INF, NAN, 2.0, 7.0), A(0.0, 0.0, SE, SE), A(-INF, NAN, INF, 7.0)
    ex = np.array([False, False, False, True])
    n = len(RP.TABLE)
    assert RP.measure("c", "o", A(-INF, NAN, 2.0 + E, NAN), want, mag, comp, ex) == 0.5         # the composition's inf: its term dropped
    assert len(RP.TABLE) == n + 1 and RP.WORST["o"] == (0.5, RP.TABLE[n])
    refused(RP.measure, "c", "o", A(INF, NAN, 2.0, 7.0), want, mag, comp, ex)
    refused(RP.measure, "c", "o", A(-3e38, NAN, 2.0, 7.0), want, mag, comp, ex)
    refused(RP.measure, "c", "o", A(-INF, 0.0, 2.0, 7.0), want, mag, comp, ex)
    refused(RP.measure, "c", "o", A(-INF, NAN, INF, 7.0), want, mag, comp, ex)
    refused(RP.measure, "c", "o", A(-INF, NAN, 2.0, NAN), want, mag, comp)                      # not excluded: 7.0 is to be met
    over_the_tolerance(RP.measure, "c", "o", A(-INF, NAN, 0.5 + 2 * RP.TOL, 7.0), A(-INF, NAN, 0.5, 7.0), A(0.0, 0.0, HUGE, SE), comp, ex)   # TOL * max(1, .)
    n = len(RP.TABLE)
    assert RP.measure("c", "o", A(-INF, NAN), A(-INF, NAN), A(0.0, 0.0), A(0.0, 0.0)) == 0.0 and len(RP.TABLE) == n


def test_losses_slices_and_the_scale_before_slicing():
    want, mag = A(1.0, 2.0, 1024.0), A(SE, SE, SE)
    first = np.array([True, True, False])
    n = len(LP.TABLE)
    assert LP.measure("k", "g", "c", A(1.0, 2.0 + E, 1024.0), want, mag) == 0.5                 # comp=None: the derived term alone
    assert LP.measure("k", "g", "c", A(1.0, 2.0 + E, 1024.0), want, mag, A(1.0, 2.0 + E / 2, INF), first) == 0.25
    w = LP.WORST[("k", "g")]
    assert len(LP.TABLE) == n + 2 and w == dict(ratio=0.5, rel=E / 2, comp_ratio=0.25, comp_rel=E / 4, line=LP.TABLE[n])
    refused(LP.measure, "k", "g", "c", A(1.0, NAN, 1024.0), want, mag)
    refused(LP.measure, "k", "g", "c", A(1.0, INF, 1024.0), want, mag, None, first)
    assert LP.measure("k", "g", "c", A(1.0, 2.0, NAN), want, mag, None, first) == 0.0           # another slice's entry
    big = A(HUGE, HUGE, SE)
    over = 2.0 + 512 * LP.TOL                                                                   # over TOL * 2, under TOL * 1024
    assert LP.measure("k", "g", "c", A(1.0, over, 1024.0), want, big, None, first) < 1.0        # the scale is the whole tensor's
    over_the_tolerance(LP.measure, "k", "g", "c", A(1.0, over, 2.0), A(1.0, 2.0, 2.0), big, None, first)
    assert LP.measure("k", "g", "c", A(1.0, over, 2.0), A(1.0, 2.0, 2.0), big, None, first, aggregate=False) < 1.0
    with pytest.raises(AssertionError):
        LP.measure("k", "g", "c", want, A(1.0, NAN, 1024.0), mag, check=False)
    assert LP.measure("k", "g", "c", A(1.0), A(1.0), A(SE), None, np.array([False])) == 0.0
