"""BASELINE config 4 (32 768 paths of N = 200, KP, obstacle corridors) on the device (GPU) — the batch bench.py times and, until this module, no test solved.

One host-pointer call on the whole batch at the headline setting (tests/test_accuracy_full.py::HEADLINE): every path solved and certified — the CPU oracle certifies all
32 768 at that setting (status 1 / status_refine 1 on every path, iterations mean 39.3, max 99), so the cap on exceptions is 0.  The 8-way contiguous split of
path_optimizer_amd.shard.shard_range, solved shard by shard, returns states, x and po_info bit-identical to the matching rows of the one-call result (4 096 and 32 768 are
both at or above the auto-slicing threshold of 2 x wave_slots, so the same kernels run: newton_parked >= 0 on both).  64 paths of shards 3 and 7 each, every 64th path of
the shard, are compared with the oracle — headline setting at the bar of test_gpu_fuzz._newton_case, OSQP-faithful default at the bar of test_ragged_batch — and 8 of
them per shard carry a solver-independent KKT certificate (np_twin.kkt_certificate) at the bars of test_gpu_fuzz.py.  The device rows of those comparisons are taken
from the ONE-CALL results, not from a separate small solve.

Measured wall time on one MI355X: the whole module 9 s — 4.8 s for the fixtures (32 768 synthetic paths and the one-call solve, 0.7 GB in and 0.5 GB out through pinned
staging), 0.2 s for the eight shards, 0.2 - 0.4 s per oracle comparison, 1.3 s for the 16 KKT certificates; well under the 30 s above which the oracle / KKT tests would
have been marked `slow`.  Measured there: 0 of 32 768 paths uncertified, iterations mean 39.13 / max 99, 31 585 paths parked by the sliced Newton launch; against the
oracle max |dx| 5.2e-8 (headline) and 5.1e-10 (OSQP-faithful, iteration counts equal on all 128 paths); KKT worst primal violation 1.8e-8, stationarity 8.9e-12."""
import numpy as np
import pytest

import np_twin as T
from path_optimizer_amd import synth
from path_optimizer_amd.shard import shard_range
from test_accuracy_full import HEADLINE

pytestmark = pytest.mark.gpu
B4, WORLD = 32768, 8
ORACLE_SHARDS = (3, 7)


def _engine(kw):
    from path_optimizer_amd import binding

    p = binding.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return binding.Engine(0, p)


def _take(b, idx):
    f = lambda a: None if a is None else np.ascontiguousarray(a[idx])
    return synth.Batch(b.formulation, len(idx), b.N, b.keep, f(b.ref_x), f(b.ref_y), f(b.ref_z), f(b.ref_k), f(b.ref_s), f(b.bounds), f(b.x0), f(b.goal_z),
                       f(b.max_k), f(b.max_kp), f(b.n_points))


def _sample(k, every=64):
    lo, hi = shard_range(B4, WORLD, k)
    return np.arange(lo, hi, every)


@pytest.fixture(scope="module")
def big():
    b = synth.make_batch(4, B=B4)
    assert (b.formulation, b.B, b.N, b.keep) == (synth.PO_KP, B4, 200, 4)
    return b


def _one_call(big, kw):
    eng = _engine(kw)
    try:
        st, info, xs = eng.solve_batch(big, want_x=True)
        dbg = (eng.debug_get("newton_parked"), eng.debug_get("newton_list_ok")) if kw.get("refine") else None
    finally:
        eng.close()  # (0.7 GB of pinned staging in, 0.5 GB out: released before anything else runs)
    return st, info, xs, dbg


@pytest.fixture(scope="module")
def one_call_headline(big):
    return _one_call(big, HEADLINE)


@pytest.fixture(scope="module")
def one_call_default(big):
    return _one_call(big, {})


def test_whole_batch_in_one_call_every_path_solved_and_certified(one_call_headline):
    st, info, xs, (parked, list_ok) = one_call_headline
    bad = np.flatnonzero((info["status"] != 1) | (info["status_refine"] != 1))
    print(f"config 4, one call: {len(bad)} of {B4} paths not solved + certified; iters mean {info['iters'].mean():.2f} max {int(info['iters'].max())}; parked {parked}")
    assert len(bad) == 0, (len(bad), bad[:16], info["status"][bad[:16]], info["status_refine"][bad[:16]])  # the oracle certifies 32 768 of 32 768
    assert info["iters"].max() <= 25 + 300
    assert parked >= 0 and list_ok == 1  # the sliced Newton launches ran, and the second launch's list was what nw_sort_kernel promises
    assert np.isfinite(st).all() and np.isfinite(xs).all()


def test_eight_way_split_is_bit_identical_to_the_one_call_result(big, one_call_headline):
    st, info, xs, (parked, _) = one_call_headline
    assert parked >= 0
    reused = None
    try:
        for k in range(WORLD):
            lo, hi = shard_range(B4, WORLD, k)
            assert (lo, hi) == (4096 * k, 4096 * (k + 1))
            eng = _engine(HEADLINE) if k < 2 or reused is None else reused  # a fresh engine for the first two shards, one reused engine for the rest
            try:
                s_st, s_info, s_xs = eng.solve_batch(big.slice(lo, hi), want_x=True)
                assert eng.debug_get("newton_parked") >= 0 and eng.debug_get("newton_list_ok") == 1, k  # sliced like the one-call solve: the same kernels ran
            finally:
                if k < 2:
                    eng.close()
                else:
                    reused = eng
            assert np.array_equal(s_st.view(np.uint64), st[lo:hi].view(np.uint64)), (k, "states", int((s_st != st[lo:hi]).any(axis=(1, 2)).sum()))
            assert np.array_equal(s_xs.view(np.uint64), xs[lo:hi].view(np.uint64)), (k, "x", int((s_xs != xs[lo:hi]).any(axis=1).sum()))
            for f in info.dtype.names:
                a, c = s_info[f], info[f][lo:hi]
                assert a.tobytes() == c.tobytes(), (k, f, np.flatnonzero(a != c)[:8])
    finally:
        if reused is not None:
            reused.close()


@pytest.mark.parametrize("k", ORACLE_SHARDS)
def test_sampled_paths_of_the_one_call_result_match_the_oracle_headline(oracle, big, one_call_headline, k):
    st, info, xs, _ = one_call_headline
    idx = _sample(k)
    assert len(idx) == 64
    po = oracle.device_equivalent_params()
    for f, v in HEADLINE.items():
        setattr(po, f, v)
    ost, oinfo, oxs = oracle.solve_batch(_take(big, idx), po, want_x=True)
    dx, ds = np.abs(xs[idx] - oxs).max(), np.abs(st[idx] - ost).max()
    print(f"shard {k} headline: max|dx| {dx:.3e} max|dstates| {ds:.3e}")
    assert np.array_equal(info["status"][idx], oinfo["status"]) and np.array_equal(info["status_refine"][idx], oinfo["status_refine"])
    assert dx < 1e-5 and ds < 1e-5, (k, dx, ds)


@pytest.mark.parametrize("k", ORACLE_SHARDS)
def test_sampled_paths_of_the_one_call_result_match_the_oracle_osqp_faithful(oracle, big, one_call_default, k):
    st, info, xs, _ = one_call_default
    idx = _sample(k)
    ost, oinfo, oxs = oracle.solve_batch(_take(big, idx), oracle.device_equivalent_params(), want_x=True)
    ok = oinfo["status"] == 1
    dx = np.abs(xs[idx] - oxs)[ok].max()
    print(f"shard {k} OSQP-faithful: {int(ok.sum())} of 64 solved; max|dx| {dx:.3e}; iters differ on {int((info['iters'][idx] != oinfo['iters']).sum())}")
    for f in ("status", "iters", "n_refactor"):
        assert np.array_equal(info[f][idx], oinfo[f]), (k, f, info[f][idx], oinfo[f])
    assert ok.any() and dx < 1e-6 and np.abs(st[idx] - ost)[ok].max() < 1e-6, (k, dx)


@pytest.mark.parametrize("k", ORACLE_SHARDS)
def test_sampled_paths_of_the_one_call_result_carry_a_kkt_certificate(oracle, big, one_call_headline, k):
    """Solver-independent: the KKT conditions of the reference's QP (oracle assembly = the reference's, bit for bit) at the device's point."""
    st, info, xs, _ = one_call_headline
    idx = _sample(k)[::8]
    assert len(idx) == 8
    pa = oracle.default_params()
    nv, _, _ = oracle.dims(big.formulation, big.N, big.keep)
    worst = [0.0, 0.0]
    for i in idx:
        assert info["status"][i] == 1 and info["status_refine"][i] == 1, int(i)
        P, A, l, u = oracle.assemble(big.formulation, pa, big.N, big.keep, big.ref_k[i], big.ref_s[i], big.ref_z[i, -1], big.bounds[i], big.x0[i], big.goal_z[i])
        c = T.kkt_certificate(P, A, l, u, xs[i, :nv])
        worst = [max(worst[0], c["primal_violation"]), max(worst[1], c["stationarity_rel"])]
        assert c["primal_violation"] < 1e-6 and c["stationarity_rel"] < 1e-5, (int(i), c)
    print(f"shard {k} KKT of the device point, worst of 8: primal violation {worst[0]:.2e} stationarity_rel {worst[1]:.2e}")
