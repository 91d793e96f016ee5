"""The smoothing-QP engine (path_optimizer_amd/csrc/po_smooth.hip) where tests/test_smooth.py does not reach: the in-loop infeasibility exit, the layouts of
QPs above 250 points (single-lane substitution under the launcher's own choice, ragged batches that mix the block's layout with the instance's), TENSION
across its factor layouts, the capacity check, every launch variant at the smallest batch that selects it, and per-instance misuse.

Every test that claims a variant or a layout asserts it through po_debug_get "smooth_variant_used" and through tests/smooth_layout.py, the Python restatement of
the layout rules, which the CPU tests of this file hold to the library.  Tolerances are test_smooth._compare's, unchanged.  The batches are small (3 - 8
instances), so iteration counts are asserted equal on EVERY instance; test_oracle_termination_margins keeps the seeds away from a termination check that
round-off could flip.

Which exits finite data can reach (read from assemble(), po_smooth.hip, and the oracle's twin of it):
  * TENSION2 (kind 0) is always primal feasible: its rows are the chain x[i+1] = x[i] + ..., y[i+1] = ..., z[i+1] = z[i] + ... plus x[0], y[0] pinned — every row
    introduces a variable no earlier row has fixed, so the chain can be walked from the pinned start for ANY data.  No inequality at all.
  * TENSION (kind 1) is always primal feasible: row 3i + 2 boxes the offset d[i] in [-c, c] with c >= 0 (a clearance, or 0 / 0.5 at the ends), rows 3i and
    3i + 1 then DEFINE x[i], y[i] from d[i]; any d inside its box is a feasible point.
  * POST (kind 2) can be primal infeasible with l <= u on every row: rows 3i + 1, 3i + 2 are the chain x[i+1] = x[i] + ds dx[i], dx[i+1] = dx[i] + ds ddx[i];
    with ds == 0 the first forces x[i+1] == x[i], and the boxes on the two (or l0 and the box of point 1) may be disjoint.  The data validation does not
    see it; the ADMM loop ends with the certificate.  That is the exit tested here.
  * No kind can be dual infeasible: that needs a direction d with P d = 0, q'd < 0 and A d inside the recession cone of [l, u].  q is zero for kinds 1 and 2,
    and for kind 0 it is non-zero only on x[i], y[i], whose Hessian diagonal 2 w_dev is positive — so q'd < 0 contradicts P d = 0.  (w_dev = 0 makes q zero too.)
So PO_STATUS_DUAL_INFEASIBLE, and PO_STATUS_PRIMAL_INFEASIBLE from the loop for kinds 0 and 1, are unreachable with finite data and are not tested."""
import ctypes as C

import numpy as np
import pytest

import smooth_layout as SL
from path_optimizer_amd import synth
from path_optimizer_amd.abi import INFO_BYTES, INFO_DTYPE, PO_ERR_UNSUPPORTED, PO_OK, PO_STATUS_PRIMAL_INFEASIBLE, PO_STATUS_SOLVED, PO_STATUS_UNSOLVED
from path_optimizer_amd.abi import PoSmoothIn, PoSmoothOut
from test_smooth import _compare, dmap, engine, omap  # noqa: F401  (dmap, engine, omap: module-scoped fixtures, one instance for this file)

KINDS = [0, 1, 2]
SWITCHES = ("smooth_waves", "smooth_nopad", "smooth_seq")

# ------------------------------------------------------------------ the sizes, as literals (what the layout rules gave when these tests were written) ...
CHUNK = {0: {64: 4, 65: 8, 129: 12, 193: 16, 257: 20, 261: 0, 262: 20, 343: 0, 344: 0},
         2: {64: 3, 65: 6, 129: 9, 256: 12, 257: 15, 321: 18, 325: 0, 326: 18, 473: 0}}
FIRST_ZEROS = {0: [261, 266, 271], 2: [325, 331, 337]}
LARGEST = {0: 344, 1: 349, 2: 473}
REFUSED_BELOW = {0: (327, 331), 2: (472, 473)}  # (a refused P below the largest admissible one, the nearest admissible P above it)
REFUSED_BYTES = {(0, 327): 165936, (0, 331): 156080}
BLOCKED_LAST = 117            # TENSION: the block layout of the factor up to here, the natural one from 118
TENSION_TWO_PER_CU_LAST = 171  # ... and two QPs per CU up to here, one from 172
LARGE = {0: [257, 260, 261, 262, 331, 344], 2: [257, 321, 325, 326, 473]}
TENSION_SWEEP = [3, 4, 5, 6, 7, 9, 10, 115, 116, 117, 118, 119, 120, 171, 172, 349]
# block layout x instance layout: kind, a.P, n_points
MIXED = [(0, 262, [262, 261, 257, 193, 129, 65, 64, 3]), (0, 261, [261, 257, 129, 64, 3]), (2, 326, [326, 325, 257, 129, 65, 64, 4]), (2, 325, [325, 321, 257, 65, 4])]
# launch variants at the smallest batch that selects them: kind, P, B, 10 * waves + WPE, QPs per CU by LDS
VARIANTS = [(0, 100, 513, 43, 3), (1, 60, 513, 43, 3), (2, 110, 513, 43, 3), (0, 100, 512, 42, 3), (1, 60, 512, 42, 3), (2, 110, 512, 42, 3),
            (0, 40, 769, 11, 8), (1, 30, 769, 11, 6), (2, 60, 769, 11, 7), (0, 40, 768, 43, 8), (1, 30, 768, 43, 6), (2, 60, 768, 43, 7)]


# ------------------------------------------------------------------ ... and derived from the rules (test_size_tables_follow_from_the_layout_rules holds the two together)
def _admissible(kind):
    return [P for P in range(SL.MINP[kind], 601) if SL.fits(kind, P)]


def _derived_large(kind):
    adm = _admissible(kind)
    zero = next(P for P in adm if SL.chunk(kind, P) == 0)  # the first size that runs the single-lane substitution by the launcher's own choice
    top = SL.chunk(kind, zero - 1)                          # the chunk length below it
    first = lambda c: next(P for P in adm if SL.chunk(kind, P) == c)
    if kind == 0:
        return [first(top), zero - 1, zero, zero + 1, _derived_refused(0)[1], adm[-1]]
    return [first(top - SL.W[2]), first(top), zero, zero + 1, adm[-1]]  # (top - W = 15: odd, the wkp copy carries no dead double; top = 18: even)


def _derived_refused(kind):
    """Kind 0: the first refused P whose admissible neighbour above is more than one step away (a refused RUN); kind 2: the last refused P below the largest."""
    adm = set(_admissible(kind))
    holes = [P for P in range(SL.MINP[kind], max(adm)) if P not in adm]
    if kind == 0:
        P = next(P for P in holes if P - 1 in adm and P - 2 in adm and P + 1 not in adm and P + 2 not in adm and P + 3 not in adm)
    else:
        P = holes[-1]
    return P, next(Q for Q in range(P, max(adm) + 1) if Q in adm)


def _tension_sweep():
    last_blocked = max(P for P in _admissible(1) if SL.blocked(1, P))
    last_two = max(P for P in _admissible(1) if SL.by_lds(1, P) >= 2)
    small = [P for P in range(3, 11) if P != 8]  # n = 9 (one block of 9 columns) ... 30 (just past three); 8 left out: 24 columns, the same case as 7 and 9
    return small + [last_blocked + d for d in (-2, -1, 0, 1, 2, 3)] + [last_two, last_two + 1, _admissible(1)[-1]]


# ------------------------------------------------------------------ inputs (shared by the CPU margin check and the GPU tests) and the oracle's results, computed once
# Seeds: 900 + 7 * kind + P unless test_oracle_termination_margins refuses that batch (chosen on the CPU, from the oracle alone):
#   TENSION P = 117: instance 0 of seed 1024 reaches r_prim = 2.4e-9 before its one rho update, so the new rho is a ratio of round-off — the oracle's own rho
#       moves by 1.2e-3 when its inputs move by an ulp, and the device (iterates within 1e-7, same iteration counts) reported 24.22 against the oracle's 24.30, which
#       _compare's rtol of 1e-4 on rho rightly refuses to call equal.  The one seed of this file that a GPU run made us look at.
#   TENSION P = 349 and P = 60 (the 16 instances of the variant tests): an ulp on the inputs moves the oracle's iterates by 2.4e-8 and 5.1e-8 — too close to the
#       1e-7 the device is held to.  (The device passed on both; replaced all the same, so that every batch here meets one criterion.)
# No seed was replaced because of a flipped termination check.
SEEDS = {(1, 117): 2117, (1, 349): 2349, (1, 60): 2060}


def _seed(kind, P):
    return SEEDS.get((kind, P), 900 + 7 * kind + P)


def _batch(kind, P, B=3, n_points=None):
    inp = synth.make_smooth_inputs(_seed(kind, P), B, P=P, kind=kind, jitter_ds=True)
    if n_points is not None:  # ragged by hand: the first n_points of a full-length instance
        inp["n_points"] = np.asarray(n_points, dtype=np.int32)
    return inp


def _infeasible_batch(P):
    """synth batch 23 of POST QPs with instance 2 and instance 4 made infeasible behind rows that all have l <= u: a repeated s forces x[i+1] == x[i]."""
    base = synth.make_smooth_inputs(23, 6, P=P, kind=2)
    inp = {k: (None if v is None else v.copy()) for k, v in base.items()}
    inp["s"][2, 1] = inp["s"][2, 0]               # x[1] == x[0] == l0 ...
    inp["l0"][2] = inp["ub"][2, 1] + 0.7          # ... which lies above the box of point 1
    inp["s"][4, 11] = inp["s"][4, 10]             # x[11] == x[10] ...
    inp["lb"][4, 10], inp["ub"][4, 10] = -1.0, -0.5
    inp["lb"][4, 11], inp["ub"][4, 11] = 0.5, 1.0  # ... with disjoint boxes
    return base, inp


def _cases():
    """name -> (kind, inputs): every batch the GPU tests of this file compare with the oracle."""
    c = {}
    for P in (30, 130):
        c[f"infeasible-{P}"] = (2, _infeasible_batch(P)[1])
    for kind in (0, 2):
        for P in LARGE[kind]:
            c[f"large-{kind}-{P}"] = (kind, _batch(kind, P))
    for kind, P, npts in MIXED:
        c[f"mixed-{kind}-{P}"] = (kind, _batch(kind, P, B=len(npts), n_points=npts))
    for P in TENSION_SWEEP:
        c[f"tension-{P}"] = (1, _batch(1, P))
    for kind, P in sorted({(k, P) for k, P, _, _, _ in VARIANTS}):
        c[f"variant-{kind}-{P}"] = (kind, _batch(kind, P, B=16))
    return c


_CASES, _ORACLE = {}, {}


def _case(name):
    if not _CASES:
        _CASES.update(_cases())
    return _CASES[name]


def _oracle_of(oracle, omap, name):
    if name not in _ORACLE:
        kind, inp = _case(name)
        _ORACLE[name] = oracle.smooth_batch(kind, oracle.default_params(), inp, m_map=omap, want_raw=True)
    return _ORACLE[name]


def _lib():
    from path_optimizer_amd import binding

    L = binding.lib()
    L.po_smooth_lds_bytes.restype = C.c_size_t
    L.po_smooth_lds_bytes.argtypes = [C.c_int, C.c_int]
    L.po_smooth_blocked.argtypes = [C.c_int, C.c_int]
    return L


# ------------------------------------------------------------------ CPU
def test_layout_helper_matches_library():
    L = _lib()
    for kind in KINDS:
        for P in range(SL.MINP[kind], 601):
            assert SL.lds_bytes(kind, P) == L.po_smooth_lds_bytes(kind, P), (kind, P)
            assert SL.blocked(kind, P) == L.po_smooth_blocked(kind, P), (kind, P)


def test_size_tables_follow_from_the_layout_rules():
    """The sizes the GPU tests run are the ones the layout rules single out.  A change of the rules fails here: derive the tables again and look at the tests."""
    L = _lib()
    for kind in (0, 2):
        assert {P: SL.chunk(kind, P) for P in CHUNK[kind]} == CHUNK[kind]
        adm = _admissible(kind)
        assert [P for P in adm if SL.chunk(kind, P) == 0][:3] == FIRST_ZEROS[kind]
        assert not [P for P in range(SL.MINP[kind], FIRST_ZEROS[kind][0]) if SL.chunk(kind, P) == 0 or not SL.fits(kind, P)]  # small QPs: always partitioned, always admitted
        assert _derived_large(kind) == LARGE[kind]
        assert _derived_refused(kind) == REFUSED_BELOW[kind]
        for P in LARGE[kind]:
            assert SL.by_lds(kind, P) == 1 and SL.variant(kind, P, 3) == 100 * kind + 82
        bad, good = REFUSED_BELOW[kind]
        assert L.po_smooth_lds_bytes(kind, bad) > SL.LDS_PER_CU >= L.po_smooth_lds_bytes(kind, good) and bad < good <= LARGEST[kind]
    for (kind, P), b in REFUSED_BYTES.items():
        assert L.po_smooth_lds_bytes(kind, P) == b
    for kind in KINDS:  # the capacity: the largest admissible P, the first one above it refused
        assert _admissible(kind)[-1] == LARGEST[kind]
        assert L.po_smooth_lds_bytes(kind, LARGEST[kind]) <= SL.LDS_PER_CU < L.po_smooth_lds_bytes(kind, LARGEST[kind] + 1)
    assert _admissible(1) == list(range(3, LARGEST[1] + 1))  # TENSION: one interval
    # TENSION's factor layout: the library decides (po_smooth_blocked), the literal follows it
    assert [L.po_smooth_blocked(1, P) for P in range(3, 601)] == [int(P <= BLOCKED_LAST) for P in range(3, 601)]
    assert max(P for P in _admissible(1) if SL.by_lds(1, P) >= 2) == TENSION_TWO_PER_CU_LAST
    assert _tension_sweep() == TENSION_SWEEP
    assert sorted({P % 3 for P in TENSION_SWEEP if BLOCKED_LAST - 3 < P <= BLOCKED_LAST}) == sorted({P % 3 for P in TENSION_SWEEP if BLOCKED_LAST < P <= BLOCKED_LAST + 3}) == [0, 1, 2]
    # block layout x instance layout: the block of a.P pads (or not), and the batch holds instances of every chunk class, among them ones that would pad alone
    for kind, P, npts in MIXED:
        own = [SL.chunk(kind, n) for n in npts]
        assert npts[0] == P and (SL.chunk(kind, P) >= 6) == (P in (262, 326))
        assert any(c >= 6 for c in own[1:]) and any(0 < c < 6 for c in own) and (SL.chunk(kind, P) == 0 or 0 in own)
    # launch variants: each batch size is the smallest (largest) that selects its variant
    for kind, P, B, v, q in VARIANTS:
        assert SL.by_lds(kind, P) == q and SL.variant(kind, P, B) == 100 * kind + v, (kind, P, B)
        assert SL.variant(kind, P, B - 1 if B in (513, 769) else B + 1) != 100 * kind + v
        assert SL.n_of(kind, P) < 256 or B > SL.CUS


def test_chunk_of_float_expression_is_exact():
    """Prob::chunk_of: (int)((j + 0.5f) * (1.0f / cch)) == j / cch in float32, for every padded chunk length any admissible size of kinds 0 and 2 produces and
    every column index the kernel forms (j < np + 8)."""
    for kind in (0, 2):
        reach = {}  # cch -> the largest np it is used with
        for P in _admissible(kind) + list(range(LARGEST[kind] + 1, 901)):  # (and beyond the capacity: room for a larger tile)
            c = SL.chunk(kind, P)
            if c >= 6:
                reach[c] = max(reach.get(c, 0), SL.n_of(kind, P) + SL.col_pad(SL.W[kind]))
        assert min(reach) == 6 + 2 * (kind == 0) and len(reach) >= 5
        for c, np_ in reach.items():
            j = np.arange(np_ + 8)
            got = ((j.astype(np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(c))).astype(np.int64)
            assert np.array_equal(got, j // c), (kind, c)


def _infeasible_expected():
    return [PO_STATUS_SOLVED, PO_STATUS_SOLVED, PO_STATUS_PRIMAL_INFEASIBLE, PO_STATUS_SOLVED, PO_STATUS_PRIMAL_INFEASIBLE, PO_STATUS_SOLVED]


@pytest.mark.parametrize("P", [30, 130])
def test_oracle_post_infeasible_certificates(oracle, P):
    base, inp = _infeasible_batch(P)
    for b in (2, 4):  # not the l > u case of the data validation
        _, _, _, l, u = oracle.smooth_assemble(2, oracle.default_params(), inp, b)
        assert (l <= u).all()
    ox, _, _, info, raw = _oracle_of(oracle, None, f"infeasible-{P}")
    bx, _, _, binfo, braw = oracle.smooth_batch(2, oracle.default_params(), base, want_raw=True)
    assert info["status"].tolist() == _infeasible_expected() and (binfo["status"] == PO_STATUS_SOLVED).all()
    bad, ok = [2, 4], [0, 1, 3, 5]
    assert (info["iters"][bad] > 0).all() and (info["iters"][bad] < oracle.default_params().max_iter).all()  # left the loop with the certificate
    assert (np.abs(raw[bad]).max(axis=1) > 0.1).all() and (np.abs(ox[bad]).max(axis=1) > 0.1).all()        # the last iterate is written, not zeros
    assert np.array_equal(raw[ok], braw[ok]) and np.array_equal(ox[ok], bx[ok]) and np.array_equal(info[ok], binfo[ok])


@pytest.mark.parametrize("name", sorted(_cases()))
def test_oracle_termination_margins(oracle, omap, name):
    """No termination check of these batches is within 2e-6 (relative) of its threshold: with every eps scaled by 1 + 2e-6 and by 1 - 2e-6 the oracle stops at the
    same iteration on every instance (the iterates do not depend on eps, only the checks do).  So a device whose residuals agree with the oracle's to round-off
    must report the same iteration counts, and the GPU tests assert exactly that."""
    kind, inp = _case(name)
    nominal = _oracle_of(oracle, omap, name)[3]
    for f in (1 + 2e-6, 1 - 2e-6):
        p = oracle.default_params()
        for key in ("eps_abs", "eps_rel", "eps_prim_inf", "eps_dual_inf"):
            setattr(p, key, getattr(p, key) * f)
        info = oracle.smooth_batch(kind, p, inp, m_map=omap)[3]
        assert np.array_equal(info["iters"], nominal["iters"]) and np.array_equal(info["status"], nominal["status"]), (f, info["iters"], nominal["iters"])
    assert (nominal["iters"] < oracle.default_params().max_iter).all()
    # ... and what _compare holds to 1e-4 (rho) and 1e-7 (the iterates) is defined that well: inputs moved by an ulp (1e-14 relative) move the oracle's own rho by
    # less than 1e-5 and its iterates by less than 1e-8.  (rho is re-estimated from a ratio of residuals: where an instance's primal residual is at round-off when
    # the estimate is taken, the ratio is noise — see _seed.)
    moved = {k: (None if v is None else v.copy()) for k, v in inp.items()}
    for key, f in (("x", 1 + 1e-14), ("y", 1 - 1e-14)) if kind < 2 else (("s", 1 + 1e-14), ("l0", 1 - 1e-14)):
        moved[key] = moved[key] * f
    other = oracle.smooth_batch(kind, oracle.default_params(), moved, m_map=omap, want_raw=True)
    assert np.array_equal(other[3]["iters"], nominal["iters"])
    assert np.abs(other[3]["rho"] / nominal["rho"] - 1).max() < 1e-5 and np.abs(other[4] - _oracle_of(oracle, omap, name)[4]).max() < 1e-8


# ------------------------------------------------------------------ GPU
def _run(engine, kind, inp, **sw):
    """One host-entry call under the given developer switches: (out_x, out_y, out_s, info, raw), and the variant the launcher picked."""
    try:
        for k in SWITCHES:
            engine.debug_set(k, sw.get(k, 0))
        res = engine.smooth_batch(kind, inp, want_raw=True)
        return res, engine.debug_get("smooth_variant_used")
    finally:
        for k in SWITCHES:
            engine.debug_set(k, 0)


def _same_bits(a, b):
    return all(np.array_equal(a[i], b[i]) for i in (0, 1, 2, 4)) and all(np.array_equal(a[3][f], b[3][f]) for f in ("status", "iters", "n_refactor", "r_prim", "r_dual", "rho", "obj"))


def _against_oracle(kind, dev, orc, inp, **kw):
    assert np.array_equal(dev[3]["iters"], orc[3]["iters"]), (dev[3]["iters"], orc[3]["iters"])  # every instance (_compare alone would allow one in ten to differ)
    return _compare(kind, dev, orc, inp, **kw)


def _zero_beyond(dev, inp):
    for b, n in enumerate(inp["n_points"]):
        assert not dev[0][b, n:].any() and not dev[1][b, n:].any() and not dev[2][b, n:].any()


@pytest.mark.gpu
def test_variant_getter_before_any_call():
    from path_optimizer_amd import binding

    e = binding.Engine(0)
    assert e.debug_get("smooth_variant_used") == 0
    e.smooth_batch(2, synth.make_smooth_inputs(1, 2, P=20, kind=2))
    assert e.debug_get("smooth_variant_used") == SL.variant(2, 20, 2) == 242


@pytest.mark.gpu
@pytest.mark.parametrize("P", [30, 130])
def test_device_post_infeasible_certificate_from_the_loop(engine, oracle, P):
    """POST QPs that are infeasible behind valid rows (l <= u everywhere): the ADMM loop ends with the primal certificate (po_smooth.hip, the exit
    `if (prim_inf)` and the certificate test above it) at the oracle's iteration, the last iterate is written like the oracle's; P = 130: chunk-padded layout."""
    _, inp = _infeasible_batch(P)
    orc = _oracle_of(oracle, None, f"infeasible-{P}")
    dev, v = _run(engine, 2, inp)
    assert v == SL.variant(2, P, 6) == (242 if P == 30 else 282)
    assert (SL.chunk(2, P) >= 6) == (P == 130)
    assert dev[3]["status"].tolist() == _infeasible_expected() == orc[3]["status"].tolist()
    assert (dev[3]["iters"][[2, 4]] > 0).all() and np.abs(dev[0][[2, 4]]).max() > 0.1
    _against_oracle(2, dev, orc, inp)
    for waves, want in ((1, 211), (4, 242), (8, 282)):
        other, v = _run(engine, 2, inp, smooth_waves=waves)
        assert v == want and _same_bits(other, dev), waves


@pytest.mark.gpu
@pytest.mark.parametrize("kind,P", [(k, P) for k in (0, 2) for P in LARGE[k]])
def test_device_large_qp_layouts(engine, oracle, omap, kind, P):
    """One QP per CU, eight waves: the last chunk lengths of the partitioned substitution and the sizes whose chunks would overrun the zero padding — there lane 0
    of the block runs band_solve alone, by the launcher's own choice (no "smooth_seq")."""
    name = f"large-{kind}-{P}"
    inp = _case(name)[1]
    dev, v = _run(engine, kind, inp)
    assert v == 100 * kind + 82 and SL.chunk(kind, P) == CHUNK[kind].get(P, SL.chunk(kind, P))
    assert (dev[3]["status"] == PO_STATUS_SOLVED).all()
    _against_oracle(kind, dev, _oracle_of(oracle, omap, name), inp)
    one, v1 = _run(engine, kind, inp, smooth_waves=1)
    assert v1 == 100 * kind + 11 and _same_bits(one, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,P,npts", MIXED)
def test_device_block_layout_times_instance_layout(engine, oracle, omap, kind, P, npts):
    """The block's a.P decides whether the LDS block carries the chunk padding, the instance's own n its chunk length: padded and unpadded blocks, each holding
    instances of every chunk class (single-lane, natural, padded with even and odd chunks)."""
    name = f"mixed-{kind}-{P}"
    inp = _case(name)[1]
    dev, v = _run(engine, kind, inp)
    assert v == 100 * kind + 82
    assert (dev[3]["status"] == PO_STATUS_SOLVED).all()
    _against_oracle(kind, dev, _oracle_of(oracle, omap, name), inp)
    _zero_beyond(dev, inp)
    one, v1 = _run(engine, kind, inp, smooth_waves=1)
    assert v1 == 100 * kind + 11 and _same_bits(one, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("P", TENSION_SWEEP)
def test_device_tension_sizes(engine, oracle, omap, P):
    """TENSION (W = 9) from one block of 9 columns to the capacity: the first blocks, both sides of the change of factor layout (all residues of P mod 3: whole and
    partial last blocks), both sides of two -> one QP per CU (four -> eight waves), the largest size."""
    name = f"tension-{P}"
    inp = _case(name)[1]
    orc = _oracle_of(oracle, omap, name)
    blocked = P <= BLOCKED_LAST
    dev, v = _run(engine, 1, inp)
    assert v == SL.variant(1, P, 3) == (182 if 3 * P >= 256 else 142)
    assert (dev[3]["status"] == PO_STATUS_SOLVED).all()
    _against_oracle(1, dev, orc, inp, blocked=blocked)
    if blocked:  # the column-by-column substitution on the natural layout
        seq, v = _run(engine, 1, inp, smooth_seq=1)
        assert v == SL.variant(1, P, 3)
        _against_oracle(1, seq, orc, inp, blocked=False)


def _prefilled(kind, P, B, fill):
    n = SL.n_of(kind, P)
    return [np.full((B, P), fill), np.full((B, P), fill), np.full((B, P), fill), np.full(B * INFO_BYTES, 0x5A, dtype=np.uint8), np.full((B, n), fill)]


def _host_call(engine, kind, inp, outs):
    """po_smooth_batch on caller-owned output arrays: the return code."""
    from path_optimizer_amd import binding

    f = lambda k: None if inp.get(k) is None else np.ascontiguousarray(inp[k], dtype=np.float64)
    arr = [f(k) for k in ("x", "y", "angle", "k", "s", "lb", "ub", "l0")]
    npts = None if inp.get("n_points") is None else np.ascontiguousarray(inp["n_points"], dtype=np.int32)
    B, P = inp["s"].shape
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    si = PoSmoothIn(kind, B, P, p(npts), *[p(a) for a in arr])
    so = PoSmoothOut(*[p(a) for a in outs])
    return binding.lib().po_smooth_batch(engine._h, C.byref(si), C.byref(so))


def _device_call(engine, kind, inp, fill=0.0, want=("x", "y", "s", "raw")):
    """po_smooth_batch_device on torch tensors pre-filled with `fill`: (return code, outputs as numpy: x, y, s, info, raw; None where not passed)."""
    import torch
    from path_optimizer_amd import binding

    B, P = inp["s"].shape
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in inp.items() if v is not None}
    out = {k: torch.full((B, SL.n_of(kind, P) if k == "raw" else P), fill, dtype=torch.float64, device="cuda") for k in want}
    out["info"] = torch.full((B, INFO_BYTES), 0x5A, dtype=torch.uint8, device="cuda")
    q = lambda d, k: None if d.get(k) is None else C.c_void_p(d[k].data_ptr())
    si = PoSmoothIn(kind, B, P, q(t, "n_points"), *[q(t, k) for k in ("x", "y", "angle", "k", "s", "lb", "ub", "l0")])
    so = PoSmoothOut(q(out, "x"), q(out, "y"), q(out, "s"), q(out, "info"), q(out, "raw"))
    rc = binding.lib().po_smooth_batch_device(engine._h, C.byref(si), C.byref(so))
    torch.cuda.synchronize()
    g = lambda k: None if k not in out else out[k].cpu().numpy()
    return rc, (g("x"), g("y"), g("s"), out["info"].cpu().numpy().reshape(-1).view(np.dtype(INFO_DTYPE)), g("raw"))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_device_capacity_is_refused_without_a_write(engine, kind):
    """The first P above the largest admissible one, and (kinds 0 and 2, whose footprint is not monotone in P) a refused P BELOW it: PO_ERR_UNSUPPORTED from both
    entries, no output touched, the variant read-back unchanged; the admissible neighbour solves."""
    refused = [LARGEST[kind] + 1] + ([REFUSED_BELOW[kind][0]] if kind != 1 else [])
    engine.smooth_batch(2, synth.make_smooth_inputs(1, 2, P=20, kind=2))
    assert engine.debug_get("smooth_variant_used") == 242
    for P in refused:
        inp = synth.make_smooth_inputs(5, 1, P=P, kind=kind)
        outs = _prefilled(kind, P, 1, 7.0)
        assert _host_call(engine, kind, inp, outs) == PO_ERR_UNSUPPORTED
        assert all((a == 7.0).all() for a in outs[:3] + outs[4:]) and (outs[3] == 0x5A).all()
        rc, dev = _device_call(engine, kind, inp, fill=7.0)
        assert rc == PO_ERR_UNSUPPORTED
        assert all((dev[i] == 7.0).all() for i in (0, 1, 2, 4)) and (dev[3].view(np.uint8) == 0x5A).all()
        assert engine.debug_get("smooth_variant_used") == 242
    if kind != 1:  # (the largest sizes themselves: test_device_large_qp_layouts, test_device_tension_sizes)
        P = REFUSED_BELOW[kind][1]
        res, v = _run(engine, kind, synth.make_smooth_inputs(5, 1, P=P, kind=kind))
        assert v == 100 * kind + 82 and res[3]["status"][0] == PO_STATUS_SOLVED


@pytest.mark.gpu
@pytest.mark.parametrize("kind,P,B,v,q", VARIANTS)
def test_device_launch_variants_at_their_thresholds(engine, oracle, omap, kind, P, B, v, q):
    """Each of <KIND, 4, 3> (the 168-register build), <KIND, 4, 2> and the automatic <KIND, 1, 1> at the batch size where the launcher starts (stops) picking it:
    16 instances repeated to B give, in every copy, the bits of the 16-instance run, which is held to the oracle."""
    name = f"variant-{kind}-{P}"
    base = _case(name)[1]
    small, v16 = _run(engine, kind, base)
    assert v16 == SL.variant(kind, P, 16) and v16 % 100 in (42, 82)
    _against_oracle(kind, small, _oracle_of(oracle, omap, name), base)
    idx = np.arange(B) % 16
    rep = {k: (None if a is None else a[idx]) for k, a in base.items()}
    big, vb = _run(engine, kind, rep)
    assert SL.by_lds(kind, P) == q and vb == 100 * kind + v
    assert _same_bits(big, tuple(a[idx] for a in small))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_device_instance_misuse_is_flagged_per_instance(engine, kind):
    """n_points below the kind's minimum or above P inside a batch (neither entry screens n_points): those instances come back PO_STATUS_UNSOLVED with zero rows,
    the others as in the clean batch."""
    P = 40
    clean = synth.make_smooth_inputs(60, 6, P=P, kind=kind, ragged=True)
    bad = {k: (None if a is None else a.copy()) for k, a in clean.items()}
    bad["n_points"][1], bad["n_points"][4] = SL.MINP[kind] - 1, P + 1
    keep = [0, 2, 3, 5]
    want = ("x", "raw") if kind == 2 else ("x", "y", "s", "raw")
    ref, _ = _run(engine, kind, clean)
    host, _ = _run(engine, kind, bad)
    rc0, dref = _device_call(engine, kind, clean, fill=7.0)
    rc1, dev = _device_call(engine, kind, bad, fill=7.0)
    assert rc0 == rc1 == PO_OK
    assert (ref[3]["status"] == PO_STATUS_SOLVED).all()
    assert np.array_equal(dref[0], ref[0]) and np.array_equal(dref[3], ref[3]) and np.array_equal(dref[4], ref[4])  # the two entries agree
    for res in (host, dev):
        assert (res[3]["status"][[1, 4]] == PO_STATUS_UNSOLVED).all() and (res[3]["iters"][[1, 4]] == 0).all()
        for i in (0, 1, 2):
            assert res[i] is None or not res[i][[1, 4]].any()
        assert np.array_equal(res[3][keep], ref[3][keep]) and np.array_equal(res[0][keep], ref[0][keep]) and np.array_equal(res[4][keep], ref[4][keep])
        for i in (1, 2):
            assert res[i] is None or np.array_equal(res[i][keep], ref[i][keep])
    assert (dev[4][[1, 4]] == 7.0).all()  # raw of a flagged instance is not written (include/po_hip.h says so)


@pytest.mark.gpu
def test_device_post_without_y_and_s_outputs(engine):
    """POST through the device entry with out->y = out->s = NULL (smooth_args_ok admits it; the kernel's guards on both): x, info and raw as with all outputs."""
    inp = synth.make_smooth_inputs(61, 6, P=70, kind=2, ragged=True, jitter_ds=True)
    rc0, full = _device_call(engine, 2, inp, fill=7.0)
    rc1, part = _device_call(engine, 2, inp, fill=7.0, want=("x", "raw"))
    assert rc0 == rc1 == PO_OK and part[1] is None and part[2] is None
    assert (full[3]["status"] == PO_STATUS_SOLVED).all() and not full[1].any() and not full[2].any()  # (POST writes zeros to y and s where given)
    assert np.array_equal(part[0], full[0]) and np.array_equal(part[3], full[3]) and np.array_equal(part[4], full[4])
    host = engine.smooth_batch(2, inp, want_raw=True)
    assert np.array_equal(host[0], full[0]) and np.array_equal(host[4], full[4]) and np.array_equal(host[3], full[3])
    # l > u with the optional outputs absent: the data-validation exit's guards
    bad = {k: (None if a is None else a.copy()) for k, a in inp.items()}
    bad["lb"][3, 2], bad["ub"][3, 2] = 1.0, -1.0
    rc2, res = _device_call(engine, 2, bad, fill=7.0, want=("x", "raw"))
    assert rc2 == PO_OK and res[3]["status"][3] == PO_STATUS_PRIMAL_INFEASIBLE and res[3]["iters"][3] == 0 and not res[0][3].any() and not res[4][3].any()
    keep = [0, 1, 2, 4, 5]
    assert np.array_equal(res[0][keep], full[0][keep]) and np.array_equal(res[4][keep], full[4][keep])
