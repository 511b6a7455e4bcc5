"""The oracle of the DFT stage tests (tests/test_dft_stage.py on the CPU, tests/test_dft_stage_gpu.py on the GPU): what
k_dft_stage of wass_amd/csrc/spectrum.hip is launched with, an fp64 model with the kernels' structure that can be broken on
purpose, the case tables, the k-hot probes and the bounds.  Test infrastructure only: nothing here is imported by the package.

k_dft_stage is  Out[m][n] = sum_k (cos - i sin)(2 pi m k / len) In[k][n]  on a 64 x 64 x 16 tile, in four instances
(CPLX, KCONTIG): a real or complex input whose k or whose n is the contiguous axis.  Its callers:
  spec3d_run         x (F,T)   y (T,F), one product per t   t (T,F)             then k_spec_power (mirror fill of kx > nx / 2)
  wass_spec1d_welch  w (F,F)                                                    then k_w1_power (one-sided doubling)
  spat_run           x (F,T)   y (T,F)   k_spat_mul   yi (T,F)   xi (T,T)       all with a batch of frames in blockIdx.z
"""
import numpy as np

import spectrum_oracle as SO

U = 2.0 ** -24                     # unit round-off of float32
TM, TN, TK = 64, 64, 16            # the tile of k_dft_stage

INSTANCES = ((False, False), (False, True), (True, False), (True, True))      # (CPLX, KCONTIG)


# ---- the launch arithmetic ------------------------------------------------------------------------------------------------------
def _stage_plan(name, cplx, kcontig, M, N, K, batch):
    return {"stage": name, "inst": (cplx, kcontig), "M": M, "N": N, "K": K, "batch": batch,
            "grid": (-(-N // TN), -(-M // TM), batch), "nk": -(-K // TK), "rM": M % TM, "rN": N % TN, "rK": K % TK}


def plan3d(nt, ny, nx):
    """The three launches of spec3d_run."""
    nxh = nx // 2 + 1
    return [_stage_plan("x", False, True, nxh, nt * ny, nx, 1), _stage_plan("y", True, False, ny, nxh, ny, nt),
            _stage_plan("t", True, False, nt, ny * nxh, nt, 1)]


def welch_dims(n_samples, nperseg):
    """(nps, step, nseg, nf) of wass_spec1d_welch / scipy.signal.csd's defaults."""
    nps = min(int(nperseg), int(n_samples))
    nov = nps // 2
    step = nps - nov
    return nps, step, (n_samples - nov) // step, nps // 2 + 1


def plan_welch(n_series, n_samples, nperseg):
    """The one launch of wass_spec1d_welch: every segment of every series is a column."""
    nps, step, nseg, nf = welch_dims(n_samples, nperseg)
    return [_stage_plan("w", False, False, nf, n_series * nseg, nps, 1)]


def plan_spatial(rows, cols, batch):
    """The four launches of spat_run."""
    ch = cols // 2 + 1
    return [_stage_plan("x", False, True, ch, rows, cols, batch), _stage_plan("y", True, False, rows, ch, rows, batch),
            _stage_plan("yi", True, False, rows, ch, rows, batch), _stage_plan("xi", True, True, cols, rows, ch, batch)]


def describe(plan):
    return "; ".join(f"{s['stage']} <{'T' if s['inst'][0] else 'F'},{'T' if s['inst'][1] else 'F'}> M {s['M']} N {s['N']} K {s['K']} grid "
                     f"{s['grid']} nk {s['nk']} ragged {s['rM']}/{s['rN']}/{s['rK']}" for s in plan)


# ---- the case tables ------------------------------------------------------------------------------------------------------------
# (nt, ny, nx).  (3, 5, 125) is there for nxh = 63: the only way to M % 64 = 63 on the x stage and N % 64 = 63 on the y stage.
CASES_3D = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (1, 5, 1), (3, 5, 7), (4, 84, 84), (5, 64, 126), (7, 65, 128), (6, 63, 127), (16, 63, 130),
            (17, 129, 66), (33, 17, 31), (66, 20, 36), (130, 9, 10), (3, 5, 125)]
# (n_samples, nperseg, rangespan) on a 41 x 43 grid.  (33, 2, 0): 2 series of 32 segments, 64 columns (N % 64 = 0); (300, 125, 0):
# nf = 63 (M % 64 = 63).  The number of series, 1 + (2 rangespan + 1)^2, is even, so compute_spectrum never has an odd number of
# columns: N % 64 = 1 and 63 cannot occur in this instance.
CASES_WELCH = [(333, 512, 3), (40, 15, 0), (40, 16, 0), (40, 17, 1), (9, 2, 0), (9, 3, 0), (700, 127, 5), (700, 129, 5), (33, 2, 0),
               (300, 125, 0)]
WELCH_GRID = (41, 43)
# (rows, cols).  (9, 29) is there for ch = 15: K % 16 = 15 on the last stage; (5, 226) for ch = 114: eight k tiles there.
CASES_SPATIAL = [(1, 1), (1, 8), (8, 1), (2, 2), (3, 3), (5, 2), (5, 3), (63, 65), (65, 63), (64, 127), (127, 129), (129, 64), (17, 130),
                 (9, 29), (5, 226)]
SPATIAL_FRAMES, SPATIAL_BATCH = 3, 2           # one full and one ragged batch


def impulse_cube(n_samples, nperseg):
    """A cube on WELCH_GRID that is 0 except at frame nps - 1, the last sample of the first segment: 1 / WELCH_SCALE on the cells of
    even y + x and half that on the others.  The periodic Hann weight of that sample is small (5.9e-4 at nps = 129), so the noisy
    cube has almost nothing in the last k tile where K % 16 = 1; here the whole first segment of every series is that sample."""
    nps = min(int(nperseg), int(n_samples))
    cube = np.zeros((n_samples,) + WELCH_GRID, np.float32)
    y, x = np.indices(WELCH_GRID)
    cube[nps - 1] = np.where((y + x) % 2 == 0, 1.0, 0.5) / WELCH_SCALE
    return cube


def welch_series_count(rangespan):
    return 1 + (2 * rangespan + 1) ** 2


# ---- the model ------------------------------------------------------------------------------------------------------------------
STAGES_3D, STAGES_WELCH, STAGES_SPATIAL = ("x", "y", "t"), ("w",), ("x", "y", "yi", "xi")
_PER_STAGE = ("drop_k", "zero_band", "twiddle_off")
VARIANTS_3D = [f"{v}:{s}" for s in STAGES_3D for v in _PER_STAGE] + ["ky_nomirror", "f_nomirror"]
VARIANTS_WELCH = [f"{v}:{s}" for s in STAGES_WELCH for v in _PER_STAGE] + ["nyquist_odd", "nyquist_even"]
VARIANTS_SPATIAL = [f"{v}:{s}" for s in STAGES_SPATIAL for v in _PER_STAGE] + ["alone_none", "alone_all"]


def _brk(variant, stage):
    """The break of `stage` that `variant` names, or None."""
    if variant and ":" in variant:
        v, s = variant.split(":")
        assert v in _PER_STAGE
        if s == stage:
            return v
    return None


def dft_stage(Bre, Bim, axis, length, M, dtype=np.float64, brk=None):
    """One k_dft_stage along `axis` of the planes Bre, Bim (Bim None for a real input): K = the axis' length is contracted with the
    twiddle of a length-`length` transform, M outputs.  dtype float32: f32-rounded twiddles and f32 matrix products (the planes
    must then be float32).  brk: 'drop_k' leaves the last 16-wide k tile out, 'zero_band' leaves the last 16-row band of the
    output zero, 'twiddle_off' takes the twiddle of m + 1 for the rows of the last 64-row tile."""
    K = Bre.shape[axis]
    m = np.arange(M, dtype=np.int64)[:, None]
    if brk == "twiddle_off":
        m = m + (m >= TM * ((M - 1) // TM))
    ang = 2.0 * np.pi * ((m * np.arange(K, dtype=np.int64)[None, :]) % length).astype(np.float64) / float(length)
    Cm, Sm = np.cos(ang), np.sin(ang)
    if brk == "drop_k":
        Cm[:, TK * ((K - 1) // TK):] = 0.0
        Sm[:, TK * ((K - 1) // TK):] = 0.0
    Cm, Sm = Cm.astype(dtype), Sm.astype(dtype)
    br = np.moveaxis(Bre, axis, 0)
    assert br.dtype == dtype
    re = np.tensordot(Cm, br, 1)
    im = -np.tensordot(Sm, br, 1)
    if Bim is not None:
        bi = np.moveaxis(Bim, axis, 0)
        re = re + np.tensordot(Sm, bi, 1)
        im = im + np.tensordot(Cm, bi, 1)
    if brk == "zero_band":
        re[TK * ((M - 1) // TK):] = 0
        im[TK * ((M - 1) // TK):] = 0
    assert re.dtype == dtype
    return np.moveaxis(re, 0, axis), np.moveaxis(im, 0, axis)


def spectrum3d_half(xw, variant=None, dtype=np.float64):
    """(re, im) [nt][ny][nxh] after the x, y and t stages of the prepared segment xw."""
    nt, ny, nx = xw.shape
    re, im = dft_stage(np.asarray(xw, dtype), None, 2, nx, nx // 2 + 1, dtype, _brk(variant, "x"))
    re, im = dft_stage(re, im, 1, ny, ny, dtype, _brk(variant, "y"))
    return dft_stage(re, im, 0, nt, nt, dtype, _brk(variant, "t"))


def power_index(nt, ny, nx, variant=None):
    """k_spec_power's (f, ky, kx) of the half spectrum for every fftshifted (it, iy, ix), and whether the bin was read at its
    mirror image."""
    it, iy, ix = np.indices((nt, ny, nx))
    f, ky, kx = (it + nt - nt // 2) % nt, (iy + ny - ny // 2) % ny, (ix + nx - nx // 2) % nx
    mir = kx > nx // 2
    kx = np.where(mir, nx - kx, kx)
    if variant != "ky_nomirror":
        ky = np.where(mir, (ny - ky) % ny, ky)
    if variant != "f_nomirror":
        f = np.where(mir, (nt - f) % nt, f)
    return f, ky, kx, mir


def staged3d(xw, variant=None, dtype=np.float64):
    """|X|^2 of the prepared segment xw [nt][ny][nx], fftshifted, float64: what one push and finish(1.0) of a wass_spec3d gives."""
    nt, ny, nx = xw.shape
    re, im = spectrum3d_half(xw, variant, dtype)
    f, ky, kx, _ = power_index(nt, ny, nx, variant)
    re, im = re[f, ky, kx].astype(np.float64), im[f, ky, kx].astype(np.float64)
    return re * re + im * im


def mirror_pairs(nt, ny, nx):
    """(a, b): flat indices into the fftshifted S such that S[a] and S[b] are computed from the same stored coefficient (a is read
    at its mirror image, b is that image read directly)."""
    f, ky, kx, mir = power_index(nt, ny, nx)
    sh = lambda k, n: (k + n // 2) % n                         # k -> fftshifted index
    b = (sh(f, nt) * ny + sh(ky, ny)) * nx + sh(kx, nx)
    a = np.arange(nt * ny * nx).reshape(nt, ny, nx)
    return a[mir], b[mir]


def welch_columns(series, nperseg):
    """B [nps][n_series * nseg] float64: the windowed, twice centred segments as k_w1_prep lays them out (series-major), without
    its cast to f32.  series: [n_series][n_samples] float64, already scaled."""
    series = np.asarray(series, np.float64)
    nps, step, nseg, _ = welch_dims(series.shape[1], nperseg)
    w = SO.hann(nps, sym=False)
    B = np.empty((nps, series.shape[0] * nseg))
    for i, x in enumerate(series):
        d = x - x.mean()
        for s in range(nseg):
            seg = d[s * step:s * step + nps]
            B[:, i * nseg + s] = (seg - seg.mean()) * w
    return B


def welch_factors(nps, nseg, fs, variant=None):
    """k_w1_power's factor per bin: the density scaling, the mean over the segments, 2 for every bin that stands for two."""
    w = SO.hann(nps, sym=False)
    fac = np.full(nps // 2 + 1, 1.0 / (fs * float((w * w).sum())) / nseg)
    m = np.arange(nps // 2 + 1)
    nyquist = (m == nps // 2) & (nps % 2 == 0)
    if variant == "nyquist_odd" and nps % 2 == 1:             # the last bin of an odd length taken for a Nyquist bin
        nyquist = m == nps // 2
    if variant == "nyquist_even":                             # the Nyquist bin of an even length doubled like the rest
        nyquist = np.zeros(m.shape, bool)
    return fac * np.where((m != 0) & ~nyquist, 2.0, 1.0)


def staged_welch(series, fs, nperseg, variant=None, dtype=np.float64):
    """{'P': the spectrum compute_spectrum returns (mean over the series of their Welch estimates), 'X': (re, im) [nf][ncol],
    'B': the columns}.  series: [n_series][n_samples] float64, already scaled."""
    nps, step, nseg, nf = welch_dims(np.shape(series)[1], nperseg)
    B = welch_columns(series, nperseg)
    re, im = dft_stage(B.astype(dtype), None, 0, nps, nf, dtype, _brk(variant, "w"))
    re, im = re.astype(np.float64), im.astype(np.float64)
    P = (re * re + im * im).sum(axis=1) * welch_factors(nps, nseg, fs, variant) / float(np.shape(series)[0])
    return {"P": P, "X": (re, im), "B": B}


def spatial_weights(rows, cols, Hs, variant=None):
    """Hw [rows][ch] of wass_spatial_filter_create from the fftshifted transfer function Hs."""
    ch = cols // 2 + 1
    Hu = np.fft.ifftshift(np.asarray(Hs, np.float64))
    kx = np.arange(ch)
    alone = (kx == 0) | ((cols % 2 == 0) & (kx == cols // 2))
    if variant == "alone_none":
        alone = np.zeros(ch, bool)
    if variant == "alone_all":
        alone = np.ones(ch, bool)
    return Hu[:, :ch] * np.where(alone, 1.0, 2.0)[None, :] * (1.0 / (float(rows) * float(cols)))


def staged_spatial(x, Hs, variant=None, dtype=np.float64):
    """real(ifft2(fft2(x) * H)) of one frame x [rows][cols] the way spat_run computes it; Hs is the fftshifted transfer function."""
    rows, cols = x.shape
    Hw = spatial_weights(rows, cols, Hs, variant)
    re, im = dft_stage(np.asarray(x, dtype), None, 1, cols, cols // 2 + 1, dtype, _brk(variant, "x"))
    re, im = dft_stage(re, im, 0, rows, rows, dtype, _brk(variant, "y"))
    re, im = (re.astype(np.float64) * Hw).astype(dtype), (-(im.astype(np.float64) * Hw)).astype(dtype)     # k_spat_mul
    re, im = dft_stage(re, im, 0, rows, rows, dtype, _brk(variant, "yi"))
    return dft_stage(re, im, 1, cols, cols, dtype, _brk(variant, "xi"))[0]


def applies(variant, case, kind):
    """Whether the variant changes anything at this case ('3d', 'welch' with case = (n_samples, nperseg, rangespan), 'spatial')."""
    if kind == "3d":
        nt, ny, nx = case
        plan = {s["stage"]: s for s in plan3d(nt, ny, nx)}
        length = {"x": nx, "y": ny, "t": nt}
        if variant == "ky_nomirror":
            return nx > 2 and ny > 2
        if variant == "f_nomirror":
            return nx > 2 and nt > 2
    elif kind == "welch":
        nps = min(case[1], case[0])
        plan = {s["stage"]: s for s in plan_welch(welch_series_count(case[2]), case[0], case[1])}
        length = {"w": nps}
        if variant == "nyquist_odd":
            return nps % 2 == 1
        if variant == "nyquist_even":
            return nps % 2 == 0
    else:
        rows, cols = case
        plan = {s["stage"]: s for s in plan_spatial(rows, cols, SPATIAL_BATCH)}
        length = {"x": cols, "y": rows, "yi": rows, "xi": cols}
        if variant == "alone_none":
            return True
        if variant == "alone_all":
            return cols > 2
    v, s = variant.split(":")
    if kind == "3d" and case == (1, 1, 1):                    # one cell minus its own mean: the prepared segment is 0 whatever is pushed
        return False
    if v == "twiddle_off":                                    # the twiddle of row m + 1 differs only where some k >= 1 is contracted
        if kind == "welch":
            # the power of a real column loses the phase: with nps = 2 the window leaves one sample, and every bin has its modulus;
            # where the last M tile holds only the row (nps - 1) / 2 + ... = nps // 2 of an odd nps, row m + 1 is its mirror image
            nps, nf = length["w"], plan["w"]["M"]
            return nps > 2 and not (nps % 2 == 1 and (nf - 1) % TM == 0)
        return plan[s]["K"] > 1 and length[s] > 1
    return True


# ---- the prepared 3-D segment, restated -----------------------------------------------------------------------------------------
def prepare3d(seg, wt, wy, wx, datascale=1.0):
    """(prepared float32 [nt][ny][nx], flag): k_seg_cell, k_seg_mean and k_seg_window in numpy.  The cell means are float32 sums
    in frame order like the kernel's; the global mean is an fp64 sum in another order than the kernel's (exact for the probes'
    small integers)."""
    v = np.asarray(seg, np.float32) * np.float32(datascale)
    nan = np.isnan(v)
    s = np.zeros(v.shape[1:], np.float32)
    for t in range(v.shape[0]):
        s = np.where(nan[t], s, s + np.where(nan[t], np.float32(0), v[t]))
    cnt = (~nan).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        cm = np.where(cnt > 0, s / cnt.astype(np.float32), np.float32(np.nan)).astype(np.float32)
    flag = bool((cnt == 0).any())
    sd = np.where(nan, 0.0, v.astype(np.float64)).sum(axis=0)
    tot = np.where(cnt > 0, sd + (v.shape[0] - cnt).astype(np.float64) * cm.astype(np.float64), 0.0)
    mean = np.float32(float(tot.sum()) / float(v.size))
    fill = np.where(nan, cm[None], v)
    win = (np.asarray(wy, np.float64)[:, None] * np.asarray(wx, np.float64)[None, :])[None] * np.asarray(wt, np.float64)[:, None, None]
    with np.errstate(invalid="ignore"):
        r = ((fill - mean).astype(np.float64) * win).astype(np.float32)
    return np.where(np.isnan(fill), np.float32(0), r), flag


# ---- k-hot probes ---------------------------------------------------------------------------------------------------------------
def hot_positions(n):
    """0, n - 1, 15 / 16 / 17 (around the first k tile's end), the first index of the last k tile, the middle, 63 / 64 (around the
    first M tile's end), where they exist."""
    want = [0, n - 1, 15, 16, 17, TK * ((n - 1) // TK), n // 2, 63, 64]
    return sorted({p for p in want if 0 <= p < n})


def _axis_pairs(n):
    """hot_positions paired first with last, second with second last, ...: every position is used; an odd one out goes with 0."""
    p = hot_positions(n)
    if len(p) == 1:
        return [(p[0],)]
    pairs = [(p[i], p[-1 - i]) for i in range(len(p) // 2)]
    if len(p) % 2:
        pairs.append((p[0], p[len(p) // 2]))
    return pairs


def probes(nt, ny, nx):
    """The probe set of a shape: per probe the hot positions of the t, y and x windows (one or two each; the first gets the weight
    1.0, the second 0.5).  First the single-hot far corner, then two-hot probes that go through every axis' pairs."""
    out = [((nt - 1,), (ny - 1,), (nx - 1,))]
    pt, py, px = _axis_pairs(nt), _axis_pairs(ny), _axis_pairs(nx)
    for j in range(max(len(pt), len(py), len(px))):
        pr = (pt[j % len(pt)], py[j % len(py)], px[j % len(px)])
        if pr not in out:
            out.append(pr)
    return out


def probe_windows(probe, nt, ny, nx):
    wins = []
    for pos, n in zip(probe, (nt, ny, nx)):
        w = np.zeros(n)
        for p, val in zip(pos, (1.0, 0.5)):
            w[p] = val
        wins.append(w)
    return wins


def probe_cube(nt, ny, nx):
    """Small integers, -6 .. 6, that vary along every axis and in no separable way: every fp64 sum of them is exact in any order."""
    t, y, x = np.indices((nt, ny, nx))
    return ((7 * t + 3 * y + 5 * x + t * y + 2 * y * x + 3 * t * x) % 13 - 6).astype(np.float32)


def probe_cells(probe, cube):
    """[(t, y, x, d)]: the non-zero cells of the prepared segment, d the exact float32 value k_seg_window writes."""
    nt, ny, nx = cube.shape
    wt, wy, wx = probe_windows(probe, nt, ny, nx)
    mean = np.float32(float(cube.astype(np.float64).sum()) / float(cube.size))
    cells = []
    for t in probe[0]:
        for y in probe[1]:
            for x in probe[2]:
                d = np.float32(np.float64(cube[t, y, x] - mean) * ((wy[y] * wx[x]) * wt[t]))
                if d != 0:
                    cells.append((t, y, x, float(d)))
    return cells


def probe_expected(cells, nt, ny, nx):
    """|X|^2, fftshifted, fp64, of the segment whose only non-zero cells are `cells`: the sum of at most eight terms
    d e^{-2 pi i (f t / nt + ky y / ny + kx x / nx)}, each a product of three one-axis factors, evaluated directly."""
    X = np.zeros((nt, ny, nx), complex)
    ph = lambda p, n: np.exp(-2j * np.pi * ((p * np.arange(n, dtype=np.int64)) % n) / n)
    for t, y, x, d in cells:
        X += d * ph(t, nt)[:, None, None] * ph(y, ny)[None, :, None] * ph(x, nx)[None, None, :]
    return np.fft.fftshift(np.abs(X) ** 2)


PROBE_C = 41.0


def probe_bound(cells):
    """e2 = (PROBE_C 2^-24 D)^2 with D = sum |d_i| over the probe's cells, for |S - S_ref| <= 2 sqrt(S_ref e2) + e2.

    The roundings, u = 2^-24.  A product with 0 and the addition of 0 are exact, so only the hot k count.  A twiddle is the f32
    rounding of an fp64 cosine: u for the rounding and another u in case the device's cosine is one fp64 ulp off and the
    rounding falls the other way, 2 u relative.
      x   real line, at most 2 hot k: a part (re or im) is a chain of at most 2 fmas, a product passes at most 2 roundings:
          (2 + 2) u l1 per part, l1 = sum |d| of the line.  Every part is at most l1 in modulus.
      y   complex line, at most 2 hot k, 2 products each: a chain of at most 4 fmas, (2 + 4) u sum |products|, and
          sum |products| <= sum (|re| + |im|) <= sqrt(2) sum |b| <= sqrt(2) l2, l2 = sum |d| of the plane: 6 sqrt(2) u l2 of its
          own.  What came in, (dre, dim) per input, goes through |c dre + s dim| <= sqrt(dre^2 + dim^2) <= sqrt(2) 4 u l1, summed
          over the line: sqrt(2) 4 u l2.  Together sqrt(2) 10 u l2 per part.
      t   the same: 6 sqrt(2) u D of its own, and sqrt(2) (sqrt(2) 10 u l2) summed over t = 20 u D from before:
          (6 sqrt(2) + 20) u D = 28.5 u D per part, sqrt(2) times that for the complex coefficient: 40.3 u D.
    Second-order terms are below 1e-5 of that; 41 covers them.  k_spec_power squares in fp64 (2^-52).  Nothing in the constant
    depends on the axis lengths."""
    D = sum(abs(c[3]) for c in cells)
    return (PROBE_C * U * D) ** 2


def tol_of(S_ref, e2):
    return 2.0 * np.sqrt(S_ref * e2) + e2


def ratio(err, tol):
    """max err / tol; where tol is 0 an error of 0 counts as 0 and any other as infinite."""
    err, tol = np.asarray(err, np.float64), np.asarray(tol, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    return float(np.max(r))


# ---- dense inputs ---------------------------------------------------------------------------------------------------------------
def dense_windows(nt, ny, nx):
    """The symmetric Hann window of n + 2 samples without its two zeros: every cell of the segment, the last k index included,
    has a weight.  (The reference's own window is 0 at both ends, and all 0 for n = 2.)"""
    return [SO.hann(n + 2)[1:-1].copy() for n in (nt, ny, nx)]


def dense_cube_3d(case, seed=0):
    """(cube, view): make_cube(nt, ny + 3, nx + 5) with 0.5 % NaN and the strided nt x ny x nx view of it that is pushed."""
    nt, ny, nx = case
    cube = SO.make_cube(nt, ny + 3, nx + 5, seed=nt + ny + nx + seed, nan_fraction=0.005)
    return cube, cube[:, 2:2 + ny, 3:3 + nx]


def bound3d_e2(xw):
    """spectrum_oracle.bound3d's formula for one prepared segment and scale 1."""
    nt, ny, nx = xw.shape
    return ((nx + ny + nt + 6) * U * float(np.abs(np.asarray(xw, np.float64)).sum())) ** 2


SPATIAL_DU, SPATIAL_CUTOFF, SPATIAL_ORDER = 0.2, 0.6, 4
SPATIAL_WAVES = ((300.0, 0.0, 0.03, 0.02, 0.3), (250.0, 0.0, 0.21, -0.17, 1.1), (150.0, 0.0, -0.05, 0.11, 2.0))


def dense_frames_spatial(case):
    """(cube, view): SPATIAL_FRAMES frames of (rows + 2) x (cols + 3) and the strided rows x cols view that is filtered."""
    rows, cols = case
    cube = SO.make_cube(SPATIAL_FRAMES, rows + 2, cols + 3, seed=rows + 2 * cols, offset=50.0, waves=SPATIAL_WAVES)
    return cube, cube[:, 1:1 + rows, 2:2 + cols]


def delta_frames(rows, cols):
    """One frame per position: a single 1.0 at each corner and at (15, 16) and (16, 15) where they exist."""
    pos = sorted({(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)} | {p for p in ((15, 16), (16, 15)) if p[0] < rows and p[1] < cols})
    fr = np.zeros((len(pos), rows, cols), np.float32)
    for i, (r, c) in enumerate(pos):
        fr[i, r, c] = 1.0
    return fr


def pair_transfer(rows, cols, p, q):
    """The fftshifted transfer function that is 1 at the bins (p, q) and (-p, -q) and 0 elsewhere: real and even."""
    Hu = np.zeros((rows, cols))
    Hu[p % rows, q % cols] = 1.0
    Hu[-p % rows, -q % cols] = 1.0
    return np.fft.fftshift(Hu)


def injected_transfers(rows, cols):
    """{name: Hs}: all ones; one mirrored pair of bins off both axes, p != q; the columns that stand alone (kx = 0 and, for even
    cols, Nyquist)."""
    p, q = 1 % rows, 2 % cols
    out = {"ones": np.ones((rows, cols)), f"pair({p},{q})": pair_transfer(rows, cols, p, q), f"pair({p},0)": pair_transfer(rows, cols, p, 0)}
    if cols % 2 == 0:
        out[f"pair({p},{cols // 2})"] = pair_transfer(rows, cols, p, cols // 2)
    return out


def butterworth_transfer(rows, cols):
    import filter_oracle as FO
    return FO.transfer_function(rows, cols, SPATIAL_DU, SPATIAL_CUTOFF, SPATIAL_ORDER)


# ---- the per-tile criterion -----------------------------------------------------------------------------------------------------
def tile_errors(got, ref, tile=64):
    """(errors, ntiles): the Frobenius norm of got - ref per tile x tile patch of the last two axes, per t for a 3-D array."""
    d = np.asarray(got, np.float64) - np.asarray(ref, np.float64)
    if d.ndim == 2:
        d = d[None]
    ty, tx = -(-d.shape[1] // tile), -(-d.shape[2] // tile)
    pad = np.zeros((d.shape[0], ty * tile, tx * tile))
    pad[:, :d.shape[1], :d.shape[2]] = d
    e = np.sqrt((pad.reshape(d.shape[0], ty, tile, tx, tile) ** 2).sum(axis=(2, 4))).ravel()
    return e, e.size


# tile limit = bound_norm / sqrt(ntiles) * TILE_MARGIN[kind]: bound_norm is the norm-wise bound of the whole array (3-D: the
# Frobenius norm of the element-wise tolerance 2 sqrt(S_ref e2) + e2; spatial: filter_oracle.spatial_bound), so that one wrong tile
# cannot hide in the budget of the others.  TILE_MARGIN is 8 x the worst ratio  tile error / (bound_norm / sqrt(ntiles))  of this
# file's own staged model run in float32 (numpy f32 matrix products, f32-rounded twiddles) against the fp64 oracle, measured on
# the CPU over the whole case table on the inputs the GPU test uses (tests/test_dft_stage.py::test_tile_margin_is_measured
# repeats the measurement).  The factor 8 is the one tests/test_grid_dct_shapes_gpu.py grants a k-ordered fma chain over a
# blocked sum.  One constant per family, because the two norm-wise bounds are of different kinds (an l1 bound per coefficient,
# a 2-norm bound per frame) and the larger constant would blunt the other family's check.  Measured worst ratios:
#   3-D      0.0632 at (130, 9, 10); the next ones 0.0245 at (3, 5, 7), 0.0235 at (66, 20, 36), 0.0175 at (33, 17, 31), 0.0016 ... 0.011
#            elsewhere (0 where the segment has one or two cells)
#   spatial  0.00813 at (3, 3); the next ones 0.0050 at (1, 8), 0.0023 at (5, 2), 0.0001 ... 0.0022 elsewhere
TILE_MEASURED = {"3d": (0.0632, (130, 9, 10)), "spatial": (0.00813, (3, 3))}
TILE_MARGIN = {k: 8 * v[0] for k, v in TILE_MEASURED.items()}


def tile_limit(bound_norm, ntiles, kind):
    return bound_norm / np.sqrt(ntiles) * TILE_MARGIN[kind]


# ---- the Welch bound ------------------------------------------------------------------------------------------------------------
WELCH_C = 4.0
WELCH_SCALE = 2.0 ** -10


def welch_tolerance(model, fs, nperseg, n_samples):
    """Per bin: factor / n_series * sum over the columns of 2 |X| e + e^2, e = (nps + WELCH_C) 2^-24 ||x_w||_1 of the column.
    nps roundings of the fma chain, and WELCH_C = 4: the f32 rounding of the twiddle (1), one more in case the device's cosine
    is an fp64 ulp off (1), the cast of the prepared column to f32 (1), one spare for the fp64 means in another order.  The test
    scales by WELCH_SCALE, a power of two, so that x * scale is exact in float32 and the fp64 oracle sees the same series."""
    nps, step, nseg, nf = welch_dims(n_samples, nperseg)
    B, (re, im) = model["B"], model["X"]
    e = (nps + WELCH_C) * U * np.abs(B).sum(axis=0)
    mod = np.sqrt(re * re + im * im)
    n_series = B.shape[1] // nseg
    return welch_factors(nps, nseg, fs) / float(n_series) * (2.0 * mod * e[None, :] + (e * e)[None, :]).sum(axis=1)
