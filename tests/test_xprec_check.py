"""xprec_check.check_frames and assert_caps on synthetic three-body frames: the harness that holds every family to its bound must
itself fail where it should."""
import numpy as np
import pytest

import xprec_check as xk

LABELS = np.array(["left", "middle", "right"])
NOBODY = np.zeros(3, dtype=bool)


def check(errs, excluded=NOBODY, bound=10.0):
    """Two frames; the implementation's "state" is its error vector, handed through by errors=."""
    frames = [(None, None, {"labels": LABELS})] * 2
    return xk.check_frames("synthetic", frames, [np.zeros(3), np.asarray(errs, dtype=np.float64)], errors=lambda s, got, res, start: got,
                           excluded=lambda res, s: excluded, bound=lambda res: bound, carries=lambda res, s: ~NOBODY)


def test_a_body_beyond_its_bound_is_named():
    with pytest.raises(AssertionError, match=r"synthetic frame 1: bodies \[1\] \(\['middle'\]\) beyond K = \[10\.\]: \[11\.\]"):
        check([1.0, 11.0, 10.0])


def test_an_excluded_body_is_not_held_to_the_bound_and_the_lists_come_back():
    errs, excl, entry = check([1.0, 11.0, 10.0], excluded=np.array([False, True, False]))
    assert [e.tolist() for e in errs] == [[0.0, 0.0, 0.0], [1.0, 11.0, 10.0]] and excl[1].tolist() == [False, True, False]
    assert entry[0].all() and xk.worst(errs, excl) == 10.0


def test_a_nan_error_is_beyond_every_bound():
    with pytest.raises(AssertionError, match=r"bodies \[2\]"):
        check([1.0, 2.0, np.nan], bound=np.inf)


def test_the_bound_may_differ_per_body():
    per_body = np.array([10.0, 100.0, 10.0])
    check([10.0, 100.0, 10.0], bound=per_body)
    with pytest.raises(AssertionError, match=r"bodies \[0\] \(\['left'\]\) beyond K = \[10\.\]: \[50\.\]"):
        check([50.0, 50.0, 1.0], bound=per_body)


def said(*values):
    """The assertion's tuple ('synthetic', values...), whichever way numpy prints a scalar."""
    return r"\('synthetic', " + ", ".join(r"(np\.\w+\()?%s\)?" % v for v in values) + r"\)"


def caps(n, excluded, carrying, floor=20):
    x, c = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    x[list(excluded)], c[list(carrying)] = True, True
    xk.assert_caps("synthetic", [x[:n // 2], x[n // 2:]], [c[:n // 2], c[n // 2:]], floor)


def test_assert_caps_fails_on_each_condition_alone():
    caps(400, range(40), range(40, 400))                                          # 10 % excluded, none that carries: passes
    with pytest.raises(AssertionError, match=said("0\\.1025")):
        caps(400, range(41), range(41, 400))                                      # 10.25 % of all body-substeps
    with pytest.raises(AssertionError, match=said(3, 25)):
        caps(400, range(3), range(25))                                            # 3 of 25 carrying ones, 22 checked, 0.75 % of all
    with pytest.raises(AssertionError, match=said(19)):
        caps(400, (), range(19))                                                  # nothing excluded, 19 carrying ones checked


def test_assert_caps_honours_a_floor_of_zero():
    caps(400, (), (), floor=0)
    with pytest.raises(AssertionError, match=said(0)):
        caps(400, (), ())
