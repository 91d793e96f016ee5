"""The LDS layout and launch rules of the smoothing-QP engine (path_optimizer_amd/csrc/po_smooth.hip), restated in Python: col_stride, col_pad,
factor_doubles, scan_chunk, Lds<KIND>::bytes, po_smooth_blocked and launch_kind.  tests/test_smooth_edges.py checks this restatement against the library
(po_smooth_lds_bytes / po_smooth_blocked, every P up to 600) and derives its sizes from it."""
W = {0: 4, 1: 9, 2: 3}      # ST<KIND>::W
KA = {0: 3, 1: 2, 2: 3}     # ST<KIND>::KA
MINP = {0: 3, 1: 3, 2: 4}   # ST<KIND>::MINP
KKT, CHUNK_PAD, CUS, LDS_PER_CU, BLOCKED_LIMIT = 4, 72, 256, 160 * 1024, 80 * 1024


def n_of(kind, P):
    return (4 * P - 1, 3 * P, 3 * P)[kind]


def m_of(kind, P):
    return (3 * (P - 1) + 2, 3 * P, 3 * P - 2)[kind]


def col_stride(w):
    return (w + 2) & ~1


def col_pad(w):
    return 4 * w


def factor_doubles(w, np_, blocked):
    nat = np_ * col_stride(w)
    if w >= 8:
        blk = (np_ + w - 1) // w * (2 * w * w)
        return blk if blocked and blk > nat else nat
    return nat


def scan_chunk(w, n):
    c = ((n + 63) // 64 + w - 1) // w * w
    return c if c * ((n + c - 1) // c) <= n + col_pad(w) else 0


def chunk(kind, P):
    """Rows per lane of the partitioned substitution for a QP of P points (kinds 0 and 2); 0: single-lane substitution."""
    return scan_chunk(W[kind], n_of(kind, P))


def _bytes(kind, P, blocked):
    w, n, m = W[kind], n_of(kind, P), m_of(kind, P)
    np_ = n + col_pad(w)
    d = factor_doubles(w, np_, blocked) + KA[kind] * m + n + np_ + 3 * m
    if w <= 4 and scan_chunk(w, n) >= 6:
        d += CHUNK_PAD + np_ + CHUNK_PAD
    b = d * 8 + (KA[kind] * m + KKT * n) * 2 + n * 4 + m + 8
    return ((b + 15) & ~15) + 64


def blocked(kind, P):
    return int(kind == 1 and _bytes(1, P, True) <= BLOCKED_LIMIT)


def lds_bytes(kind, P):
    return _bytes(kind, P, bool(blocked(kind, P)))


def fits(kind, P):
    return lds_bytes(kind, P) <= LDS_PER_CU


def by_lds(kind, P):
    return LDS_PER_CU // lds_bytes(kind, P)


def variant(kind, P, B, waves=0):
    """launch_kind: 100 * kind + 10 * waves per QP + WPE of the instantiation a batch of B QPs of P points runs (waves: the "smooth_waves" switch)."""
    q = by_lds(kind, P)
    if waves <= 0:
        alone = q == 1 or B <= CUS
        waves = 8 if alone and n_of(kind, P) >= 256 else (4 if q <= 4 or B <= 3 * CUS else 1)
    if waves == 8:
        return 100 * kind + 82
    if waves == 4:
        return 100 * kind + (43 if q >= 3 and B > 2 * CUS else 42)
    return 100 * kind + 11
