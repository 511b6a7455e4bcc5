"""A numpy restatement of the wave-by-wave statistics ("Wave-by-wave statistics"): sequential over time, vectorised
over the cells, so that every sum runs in the specified order and every product, quotient and sum is one fp64 rounding.  No GPU.

wave_stats(z, dt, ...) returns a dict of H x W maps under the names of wass_amd.postproc.WAVE_FIELDS plus n_cross, n_waves, the
derived maps, "hist", and "H" / "T": the waves themselves, [k, row, col], NaN past a cell's last wave.

`broken` names deliberate mistakes (tests/test_wavestats.py shows that the probes of the GPU suite tell each from the
specification); the empty set is the specification:
  strict_zero   <= / > instead of < / >= at an exact zero          span_off    a wave's span reaches one sample too far
  pairwise      the mean's sum by halves instead of in order       fma_eta     eta = fma(z, datascale, -(mean * datascale))
  fma_tau       tau = fma(eta[i], 1 / (eta[i] - eta[i+1]), i)      fma_moment  the moments' sums take e * e fused
  n13_floor     n13 = Nw // 3                                      tie_later   equal heights at the cut: the later wave
  sorted_sum    the third summed from the highest wave down        tz_mean     t_z as the mean of T_k
"""
from fractions import Fraction

import numpy as np

FIELDS = ("mean", "m2", "m3", "m4", "eta_max", "eta_min", "h_mean", "h_sqmean", "h_max", "t_hmax", "t_z", "h_13", "t_13")
BROKEN = ("strict_zero", "span_off", "pairwise", "fma_eta", "fma_tau", "fma_moment", "n13_floor", "tie_later", "sorted_sum", "tz_mean")


def _fma1(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))     # exact, then one rounding to nearest even


_fma = np.vectorize(_fma1, otypes=[np.float64])


def _pairwise(rows):
    if len(rows) == 1:
        return rows[0]
    h = len(rows) // 2
    return _pairwise(rows[:h]) + _pairwise(rows[h:])


def wave_stats(z, dt, datascale=1.0, crossing="up", demean=True, hist_bins=0, hist_width=0.0, broken=()):
    broken = set(broken)
    assert broken <= set(BROKEN) and crossing in ("up", "down")
    z = np.asarray(z)
    assert z.ndim == 3 and z.dtype == np.float32
    count, H, W = z.shape
    x32 = z.reshape(count, H * W)
    n = H * W
    valid = np.isfinite(x32).all(axis=0)
    x = np.where(valid[None], x32, np.float32(0)).astype(np.float64)
    dt, ds = np.float64(dt), np.float64(datascale)
    cnt = np.float64(count)
    with np.errstate(all="ignore"):
        s = np.zeros(n)
        for t in range(count):
            s = s + x[t]
        if "pairwise" in broken:
            s = _pairwise([x[t] for t in range(count)])
        mean = s / cnt
        sub = mean if demean else np.zeros(n)
        if "fma_eta" in broken:
            eta = np.stack([_fma(x[t], ds, -(sub * ds)) for t in range(count)])
        else:
            eta = np.stack([(x[t] - sub) * ds for t in range(count)])
        s2, s3, s4 = np.zeros(n), np.zeros(n), np.zeros(n)
        emax, emin = np.full(n, -np.inf), np.full(n, np.inf)
        for t in range(count):
            e = eta[t]
            e2 = e * e
            if "fma_moment" in broken:
                s2, s3, s4 = _fma(e, e, s2), _fma(e2, e, s3), _fma(e2, e2, s4)
            else:
                s2, s3, s4 = s2 + e2, s3 + e2 * e, s4 + e2 * e2
            emax = np.where(e > emax, e, emax)
            emin = np.where(e < emin, e, emin)
        c = -eta if crossing == "down" else eta
        K = max(count // 2, 1)
        Hk, Tk = np.full((K, n), np.nan), np.full((K, n), np.nan)
        ncross = np.zeros(n, np.int64)
        tau0, taup = np.zeros(n), np.zeros(n)
        crest, trough = np.full(n, -np.inf), np.full(n, np.inf)
        cells = np.arange(n)
        for t in range(count):
            if t > 0:
                a, b = c[t - 1], c[t]
                up = (a <= 0) & (b > 0) if "strict_zero" in broken else (a < 0) & (b >= 0)
                if "span_off" in broken:
                    crest, trough = np.where(b > crest, b, crest), np.where(b < trough, b, trough)
                if "fma_tau" in broken:
                    tau = _fma(a, 1.0 / (a - b), np.float64(t - 1))
                else:
                    tau = np.float64(t - 1) + a / (a - b)
                close = up & (ncross > 0)
                k = np.where(close, ncross - 1, 0)
                Hk[k[close], cells[close]] = (crest - trough)[close]
                Tk[k[close], cells[close]] = ((tau - taup) * dt)[close]
                tau0 = np.where(up & (ncross == 0), tau, tau0)
                taup = np.where(up, tau, taup)
                ncross = ncross + up
                crest, trough = np.where(up, -np.inf, crest), np.where(up, np.inf, trough)
            crest = np.where(c[t] > crest, c[t], crest)
            trough = np.where(c[t] < trough, c[t], trough)
        nw = np.maximum(ncross - 1, 0)
        has = nw > 0
        nwf = np.where(has, nw, 1).astype(np.float64)
        sh, sh2, st = np.zeros(n), np.zeros(n), np.zeros(n)
        hmax, thmax = np.zeros(n), np.zeros(n)
        for k in range(K):
            live = k < nw
            h, tk = Hk[k], Tk[k]
            sh = np.where(live, sh + h, sh)
            sh2 = np.where(live, sh2 + h * h, sh2)
            st = np.where(live, st + tk, st)
            first = live & ((k == 0) | (h > hmax))
            hmax, thmax = np.where(first, h, hmax), np.where(first, tk, thmax)
        t_z = st / nwf if "tz_mean" in broken else ((taup - tau0) * dt) / nwf
        # the highest third: rank 0 is the highest wave, equal heights ranked in time order
        n13 = nw // 3 if "n13_floor" in broken else (nw + 2) // 3
        keyed = np.where(np.isnan(Hk), -np.inf, Hk)
        if "tie_later" in broken:
            order = (K - 1) - np.argsort(-keyed[::-1], axis=0, kind="stable")
        else:
            order = np.argsort(-keyed, axis=0, kind="stable")
        rank = np.empty_like(order)
        np.put_along_axis(rank, order, np.arange(K)[:, None].repeat(n, axis=1), axis=0)
        taken = (rank < n13[None]) & (np.arange(K)[:, None] < nw[None])
        s13h, s13t = np.zeros(n), np.zeros(n)
        for r in range(K):
            if "sorted_sum" in broken:
                k = order[r]
                live = r < n13
                s13h = np.where(live, s13h + Hk[k, cells], s13h)
                s13t = np.where(live, s13t + Tk[k, cells], s13t)
            else:
                s13h = np.where(taken[r], s13h + Hk[r], s13h)
                s13t = np.where(taken[r], s13t + Tk[r], s13t)
        n13f = np.where(n13 > 0, n13, 1).astype(np.float64)
        has13 = has & (n13 > 0)
        nan = np.float64(np.nan)
        out = {
            "mean": mean * ds, "m2": s2 / cnt, "m3": s3 / cnt, "m4": s4 / cnt, "eta_max": emax, "eta_min": emin,
            "h_mean": np.where(has, sh / nwf, nan), "h_sqmean": np.where(has, sh2 / nwf, nan), "h_max": np.where(has, hmax, nan),
            "t_hmax": np.where(has, thmax, nan), "t_z": np.where(has, t_z, nan),
            "h_13": np.where(has13, s13h / n13f, nan), "t_13": np.where(has13, s13t / n13f, nan),
        }
        for name in FIELDS:
            out[name] = np.where(valid, out[name], nan).reshape(H, W)
        n_cross = np.where(valid, ncross, -1).astype(np.int32)
        out["n_cross"] = n_cross.reshape(H, W)
        out["n_waves"] = np.where(n_cross < 0, n_cross, np.maximum(n_cross - 1, 0)).astype(np.int32).reshape(H, W)
        sigma = np.sqrt(out["m2"])
        out.update(sigma=sigma, hs_m0=4.0 * sigma, skewness=out["m3"] / (out["m2"] * sigma), kurtosis=out["m4"] / (out["m2"] * out["m2"]),
                   h_rms=np.sqrt(out["h_sqmean"]))
        live = (np.arange(K)[:, None] < nw[None]) & valid[None]
        out["H"] = np.where(live, Hk, nan).reshape(K, H, W)
        out["T"] = np.where(live, Tk, nan).reshape(K, H, W)
        out["hist"] = None
        if hist_bins > 0:
            q = np.floor(Hk[live] / np.float64(hist_width))
            b = np.where(q < hist_bins - 1, q, hist_bins - 1).astype(np.int64)
            out["hist"] = np.bincount(b, minlength=hist_bins).astype(np.uint64)
    return out
