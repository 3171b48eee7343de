"""CPU tests of the action mask's count-interval table (round 6; hope_env_upload_tables -> k_obs_pair's mask stage): the table the
LIBRARY builds (hope_debug_mask_lut, pure host code) brackets the reference's first-exceed counts (src/model/action_mask.py:166-177)
for every scan value that can fall into a bin, and the kernel's two-visit evaluation -- mirrored here in numpy, same float64
expressions -- returns the exact coarse-beam minimum or raises the tie flag whenever an entry lies within 1e-9 of the scan."""
import ctypes as C

import numpy as np
import pytest

from hope_amd import load_library
from hope_amd import tables as T
from mask_program import NB, ROW, NBEAM, NACT, NITER, UPS, exact_counts, kernel_mask_counts, unpack      # the mirror shared with test_mask_program.py
import mask_program as M


def _lut_of(t):
    ds = np.ascontiguousarray(t['dist_star'], np.float64)           # [1200][42][10]
    hb = np.ascontiguousarray(t['hull_base'], np.float64)
    out = np.zeros((NBEAM * NB + 1, ROW), np.uint16)
    sc = np.zeros(NBEAM)
    lib = load_library()
    assert lib.hope_debug_mask_lut(ds.ctypes.data, hb.ctypes.data, out.ctypes.data, sc.ctypes.data) == 0
    tab = np.maximum.accumulate(ds[::UPS], axis=2)                  # [120][42][10] prefix-maxed coarse rows
    return dict(lut=out, scale=sc, tab=tab, hb=hb, pmax=tab.max(axis=(1, 2)))


@pytest.fixture(scope='module')
def lut():
    return _lut_of(T.all_tables())


@pytest.fixture(scope='module')
def lut_quantised():
    """the coarse rows on a 0.05 m grid: the library accepts the table; bins hold up to ten (equal) entries"""
    return _lut_of(M.quantised_tables())


def test_padding_and_neutral_row(lut):
    assert (lut['lut'][:, NACT // 2:] == 0xAAAA).all() and (lut['lut'][-1] == 0xAAAA).all()
    lo, hi = unpack(lut['lut'][:-1])
    assert (lo <= hi).all() and hi.max() <= NITER
    # a useful table: most entries are decided by the bin alone
    assert (lo == hi).mean() > 0.93


def test_brackets_the_float64_counts(lut):
    """every scan value, also those on bin edges, table entries and their 1e-9 neighbourhoods"""
    _brackets(lut)


def _brackets(L):
    rng = np.random.default_rng(0)
    for i in range(NBEAM):
        lo_i = L['hb'][i] - 1e-6
        xs = [rng.uniform(L['hb'][i], L['pmax'][i] + 1e-3, 4000)]
        edges = lo_i + np.arange(NB + 1) / L['scale'][i]
        for d in (0.0, 1e-12, -1e-12, 1e-9, -1e-9, 3e-9, -3e-9):
            xs.append(edges + d)
            xs.append(L['tab'][i].ravel() + d)
        x = np.concatenate(xs)
        x = x[x >= L['hb'][i]]
        q = M.bin_value_at(L, i, x)
        act = q < NB
        # beyond the last bin every entry is <= x - 1e-9 (the beam cannot lower any count)
        assert (L['tab'][i].max() <= x[~act] - 1e-9).all()
        x, q = x[act], q[act]
        b = q.astype(np.int64)
        lo, hi = unpack(L['lut'][i * NB + b])                       # [n, 42]
        cnt = (L['tab'][i][None] <= x[:, None, None]).sum(-1)
        cnt_m = (L['tab'][i][None] <= (x - 1e-9)[:, None, None]).sum(-1)
        assert (lo <= cnt_m).all() and (cnt <= hi).all()


def test_two_visit_evaluation_is_exact_or_ties(lut):
    _two_visit(lut)


def _two_visit(L):
    rng = np.random.default_rng(1)
    n_tie = 0
    for trial in range(3000):
        kind = trial % 4
        x = L['hb'] + rng.uniform(0, 10, NBEAM)                     # nothing near
        k = rng.integers(1, 40)
        near = rng.choice(NBEAM, k, replace=False)
        x[near] = L['hb'][near] + rng.uniform(0, 1.0, k) * (L['pmax'][near] - L['hb'][near]) * 1.2
        if kind == 1:                                               # scan values ON table entries (the structural tie) and just beside them
            for i in near[:4]:
                x[i] = max(L['hb'][i], L['tab'][i].ravel()[rng.integers(NACT * NITER)] + rng.choice([0.0, 5e-10, -5e-10, 2e-9, -2e-9]))
        if kind == 2:                                               # touching obstacle: the scan is the hull range itself
            x[near[:3]] = L['hb'][near[:3]]
        ms, tie = kernel_mask_counts(L, x)
        m, mlow = exact_counts(L, x), exact_counts(L, x, 1e-9)
        if (m != mlow).any():
            assert tie, 'an entry within 1e-9 of the scan must send the scene to the exact evaluation'
        if not tie:
            assert (ms == m).all()
        n_tie += tie
    assert 0 < n_tie < 3000


def test_quantised_table_is_accepted_and_keeps_both_properties(lut_quantised):
    L = lut_quantised
    lo, hi = unpack(L['lut'][:-1])
    assert (lo <= hi).all() and hi.max() <= NITER and (hi - lo).max() == NITER       # a bin that holds all ten entries of an action
    _brackets(L)
    _two_visit(L)


def _status(ds, hb):
    out = np.full((NBEAM * NB + 1, ROW), 0x1234, np.uint16)
    sc = np.full(NBEAM, -7.0)
    lib = load_library()
    ds, hb = np.ascontiguousarray(ds, np.float64), np.ascontiguousarray(hb, np.float64)
    rc = lib.hope_debug_mask_lut(ds.ctypes.data, hb.ctypes.data, out.ctypes.data, sc.ctypes.data)
    if rc != 0:
        assert (out == 0x1234).all() and (sc == -7.0).all()         # a refused table writes nothing
    return rc, lib.hope_last_error().decode(errors='replace')


@pytest.mark.parametrize('beam', [0, 37, 64, 119])
def test_a_beam_whose_table_maximum_is_not_above_its_hull_range_is_refused(beam):
    """the bin scale 128 / (max + 4e-9 - (hull_base - 1e-6)) would be negative (below) or span no scan value at all (equal): the
    kernels would index the table with (int) of a negative or unbounded number.  HOPE_EINVAL, the beam named"""
    t = T.all_tables()
    hb = t['hull_base']
    assert _status(t['dist_star'], hb)[0] == 0
    below = t['dist_star'].copy()
    below[(np.arange(10 * beam - 9, 10 * beam + 10)) % 1200] = 0.0       # the rows whose interpolation the coarse row 10 * beam enters
    rc, err = _status(below, hb)
    assert rc == -1 and f'beam {beam} ' in err, err
    equal = t['dist_star'].copy()
    equal[10 * beam] = np.minimum(equal[10 * beam], hb[beam] - 1e-6)
    assert equal[10 * beam].max() == hb[beam] - 1e-6
    rc, err = _status(equal, hb)
    assert rc == -1 and f'beam {beam} ' in err, err
    just_above = equal.copy()
    just_above[10 * beam, 3, 9] = np.nextafter(hb[beam] - 1e-6, np.inf)
    assert _status(just_above, hb)[0] == 0                          # (a positive finite scale: nothing to refuse)


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
def test_a_value_that_is_not_finite_is_refused(value):
    t = T.all_tables()
    for where in ((0, 0, 0), (775, 20, 4), (1199, 41, 9)):
        ds = t['dist_star'].copy()
        ds[where] = value
        rc, err = _status(ds, t['hull_base'])
        assert rc == -1 and f'beam {where[0] // 10} ' in err and 'dist_star' in err, err
    hb = t['hull_base'].copy()
    hb[91] = value
    rc, err = _status(t['dist_star'], hb)
    assert rc == -1 and 'beam 91' in err and 'hull_base' in err, err
