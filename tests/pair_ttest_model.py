"""The numpy restatement of illico_pair_ttest_from_moments (include/illico_hip_pair_ttest.h) for all ordered pairs: t, df, fold change
and Cohen's d, every step one IEEE float64 operation in the order the header of kernels_ttest.h writes them.  Planes are ``[K, K, W]``
indexed ``[r, g, j]``: group ``sel[g]`` against reference ``sel[r]``.  The tail (p) is not restated: it is held to the bits of
illico_ttest_from_moments on the device, and to scipy in tests/test_pair_ttest_host.py."""
import numpy as np


def pair_model(S, Q, counts, sel=None, fsum=None, overestim=False):
    """``dict(t, df, fold_change, cohen_d, t_raw)`` of float64 ``[K, K, W]`` planes from the moment planes ``S``, ``Q`` (``[G, W]``),
    the group sizes ``counts`` and the ascending group ids ``sel`` (default: all).  ``t`` is what the device writes -- a NaN t and the
    diagonal are 0 --; ``t_raw`` keeps the NaN and the diagonal's own value."""
    S, Q = np.asarray(S, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    F = S if fsum is None else np.asarray(fsum, dtype=np.float64)
    sel = np.arange(S.shape[0]) if sel is None else np.asarray(sel)
    n = np.asarray(counts, dtype=np.float64)[sel][:, None]           # [K, 1]
    S, Q, F = S[sel], Q[sel], F[sel]
    K = len(sel)
    with np.errstate(all="ignore"):
        m = S / n
        q = Q - S * m
        q = np.where(q < 0, 0.0, q)
        v = q / (n - 1.0)
        fm = F / n
        # axis 0: the reference r (side 2), axis 1: the group g (side 1)
        m1, m2, v1, v2, n1, n2 = m[None, :], m[:, None], v[None, :], v[:, None], n[None, :], n[:, None]
        n2p = np.broadcast_to(n1, (K, K, 1)) if overestim else np.broadcast_to(n2, (K, K, 1))
        a, b = v1 / n1, v2 / n2p
        t_raw = (m1 - m2) / np.sqrt(a + b)
        df = ((a + b) * (a + b)) / (a * a / (n1 - 1.0) + b * b / (n2p - 1.0))
        df = np.where(np.isnan(df), 1.0, df)
        d = (m1 - m2) / np.sqrt(0.5 * (v1 + v2))
        d = np.where(np.isnan(d), 0.0, d)
        fc = fm[None, :] / fm[:, None]
        fc = np.where(np.broadcast_to(fm[:, None] == 0.0, fc.shape), np.inf, fc)
    diag = np.eye(K, dtype=bool)[:, :, None]
    t = np.where(np.isnan(t_raw) | diag, 0.0, t_raw)
    d = np.where(diag, 0.0, d)
    return dict(t=t, df=df, fold_change=fc, cohen_d=d, t_raw=t_raw)
