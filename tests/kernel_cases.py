"""Random problem instances shared by the host-runner and GPU kernel tests."""
from __future__ import annotations

import numpy as np
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.engine.bands import DeviceBand, RecordCache, build_table, operator_table
from kafka_inferenceengine_amd.ops import kernels as K
from kafka_inferenceengine_amd.utils.blocks import pack_blocks


def spd_blocks(rng, N, n, scale=10.0):
    A = rng.normal(size=(N, n, n))
    return np.einsum("nij,nkj->nik", A, A) + scale * np.eye(n)[None]


def tip_problem(N=3000, seed=0, n_train=64, dn16=False, mask_frac=0.2):
    """7-param TIP state, 2 GP bands; returns numpy inputs + descriptors factory."""
    rng = np.random.default_rng(seed)
    ems = k.make_tip_emulators(n_train=n_train, seed=seed)
    mu, P, Pi = k.tip_prior()
    x = mu[None, :] + rng.normal(size=(N, 7)) * np.sqrt(np.diag(P)) * 0.3
    x[:, 6] = np.clip(x[:, 6], 0.05, 0.95)
    xf = mu[None, :] + rng.normal(size=(N, 7)) * 0.01
    Pf = np.broadcast_to(Pi, (N, 7, 7)) + 0.0
    specs = [k.gp_spec(ems[b], k.TIP_BAND_MAPPER[b]) for b in range(2)]
    bands_np = []
    raw = []
    for b in range(2):
        H, _ = ems[b].predict(x[:, k.TIP_BAND_MAPPER[b]])
        y = np.clip(H + rng.normal(size=N) * 0.01, 0.01, 1.0)
        valid = rng.random(N) > mask_frac
        if dn16:
            dn = np.where(valid, np.clip(np.round(y / 1e-4), 1, 65535), 0).astype(np.int32)
            yy = dn * 1e-4
            sig = np.maximum(0.05 * yy, 2.5e-3)
            w = np.where(dn > 0, 1 / sig ** 2, 0.0)
            raw.append(dict(dn=np.where(dn > 32767, dn - 65536, dn).astype(np.int16)))
            yv = np.where(dn > 0, yy, 0.0)
        else:
            w = np.where(valid, 1 / 0.01 ** 2, 0.0)
            raw.append(dict(y=y.astype(np.float32), w=w.astype(np.float32)))
            yv = y
        bands_np.append((yv, w))
    return dict(x=x, xf=xf, Pf=Pf, specs=specs, ems=ems, bands=bands_np, raw=raw, dn16=dn16, N=N, n=7)


def device_bands(prob, device):
    obs = []
    for r in prob["raw"]:
        if prob["dn16"]:
            obs.append(DeviceBand(K.OBS_DN16, dn=torch.from_numpy(r["dn"]).to(device), scale=1e-4, rel_unc=0.05,
                                  unc_floor=2.5e-3))
        else:
            obs.append(DeviceBand(K.OBS_F32, y=torch.from_numpy(r["y"]).to(device),
                                  w=torch.from_numpy(r["w"]).to(device)))
    return obs


def table(prob, device, h0_outs=None):
    return build_table(prob["specs"], device_bands(prob, device), prob["n"], RecordCache(), device, h0_outs)


def soa(a, device):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).T, dtype=np.float32)).to(device)


def packed(blocks, device):
    return torch.from_numpy(np.ascontiguousarray(pack_blocks(blocks), dtype=np.float32)).to(device)


def oracle_bands(prob, x_lin):
    out = []
    for b, (y, w) in enumerate(prob["bands"]):
        mp = k.TIP_BAND_MAPPER[b]
        H, dH = prob["ems"][b].predict(x_lin[:, mp])
        h = np.zeros((prob["N"], prob["n"]))
        h[:, mp] = dH
        out.append((H, h, y, w))
    return out


def fused_vs_materialized(device, mode, blend=False, quirk=False, prop_mask=0, N=2000, seed=3):
    """Analysis with the propagation fused into the kernel vs propagate pass +
    analysis; both linearise at the forecast (first Gauss-Newton iteration) and
    then at a perturbed point.  Returns the two (x, A, status) results."""
    from kafka_inferenceengine_amd.utils.blocks import pack_matrix
    prob = tip_problem(N=N, seed=seed)
    rng = np.random.default_rng(seed)
    n = prob["n"]
    mu, _, Pi = k.tip_prior()
    A = spd_blocks(rng, N, n, 5.0) * 0.2 + prob["Pf"]
    spec = {"mode": mode, "m": np.ones(n), "q": rng.uniform(0.01, 0.1, n), "prop_mask": prop_mask,
            "reset_mean": mu, "reset_cinv": pack_matrix(Pi), "blend": blend, "quirk_blend": quirk,
            "blend_mean": mu * 1.05, "blend_cinv": pack_matrix(Pi * 0.5)}
    xa, pa = soa(prob["x"], device), packed(A, device)
    tab = table(prob, device)
    nt = n * (n + 1) // 2
    res = []
    for fused in (False, True):
        out = []
        x_lin = None
        for it in range(2):
            xo = torch.zeros((n, N), device=device)
            ao = torch.zeros((nt, N), device=device)
            st = torch.zeros(N, dtype=torch.uint8, device=device)
            if fused:
                h = K.prop_args(n, spec, xa, pa, fused=True)
                K.analysis(n, tab, x_lin, None, None, xo, ao, None, st, None, prop=h)
            else:
                xf = torch.zeros((n, N), device=device)
                pf = torch.zeros((nt, N), device=device)
                K.propagate(n, spec, xa, pa, xf, pf)
                K.analysis(n, tab, xf if x_lin is None else x_lin, xf, pf, xo, ao, None, st, None)
            out.append((xo.cpu().numpy(), ao.cpu().numpy(), st.cpu().numpy()))
            x_lin = soa(prob["x"] * 0.5 + 0.5 * xo.cpu().numpy().T, device)
        res.append(out)
    return res


FUSED_CASES = [(1, False, False, 1 << 6), (1, False, False, 0b1010011), (0, False, False, 0),
               (2, False, False, 0)]


def tiled_vs_sequential(device, h=150, w=300, omegas=(1.0, 1.3, 1.2, 1.25, 1.22), cheb=None, n=7, j0=2, seed=5):
    """K9 temporal blocking (reg_sweeps_tiled) against one reg_sweep launch per
    sweep on a dense strip without halo rows.  Returns ((z, zp) tiled, (z, zp)
    sequential) as CPU tensors."""
    rng = np.random.default_rng(seed)
    N = h * w
    ld = N + 64
    geo = {"w": w, "h": h, "halo": 0, "n_up": 0}
    cheb = [s > 0 for s in range(len(omegas))] if cheb is None else list(cheb)
    u = torch.tensor(rng.normal(size=(n, ld)), dtype=torch.float32, device=device)
    v = torch.tensor(rng.uniform(0.0, 0.2, size=(n, ld)), dtype=torch.float32, device=device)
    z0 = torch.tensor(rng.normal(size=(1, ld)), dtype=torch.float32, device=device)
    zm1 = torch.tensor(rng.normal(size=(1, ld)), dtype=torch.float32, device=device)
    gamma, mask = 0.9, 1 << j0
    zo, zpo = (torch.zeros(1, ld, device=device) for _ in range(2))
    K.reg_sweeps_tiled(n, u, v, z0, zm1, zo, zpo, gamma, mask, N, geo, list(omegas), cheb)
    cur, prev = z0.clone(), zm1.clone()
    for om, c in zip(omegas, cheb):
        nxt = torch.zeros(1, ld, device=device)
        K.reg_sweep(n, u, v, cur, None, nxt, gamma, mask, N, geo=geo, z_prev=prev if c else None, omega=om)
        prev, cur = cur, nxt
    return (zo[:, :N].cpu(), zpo[:, :N].cpu()), (cur[:, :N].cpu(), prev[:, :N].cpu())


def deep_halo_vs_full(device, h_total=200, w=150, r0=70, r1=150, depth=8, omegas=(1.0, 1.3, 1.2, 1.25, 1.22, 1.21),
                      cheb=None, device_sched=False, split=False, n=7, j0=6, seed=11, rho=None):
    """K9 deep halo: a tiled pass over strip rows [r0, r1) of a dense raster,
    with `depth` rows of u, v, z, zp of each neighbour in halo planes (as the
    engine receives them), against the same pass over the whole raster (no
    halo).  ``device_sched``: the weights come from a RegSchedule (``rho``) and
    the pass from its table; ``split``: boundary tile rows, then the interior
    (the C2 overlap order).  Returns ((z, zp) strip, (z, zp) full rows r0..r1)."""
    rng = np.random.default_rng(seed)
    Nf = h_total * w
    ld = Nf + 32
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=device)  # noqa: E731
    u = t(rng.normal(size=(n, ld)))
    v = t(rng.uniform(0.0, 0.2, size=(n, ld)))
    z0 = t(rng.normal(size=(1, ld)))
    zm1 = t(rng.normal(size=(1, ld)))
    gamma, mask = 0.9, 1 << j0
    kw_host = {}
    if device_sched:
        rs = K.RegSchedule(Nf, 32, device)
        rs.rho.fill_(0.8 if rho is None else rho)
        rs.schedule(1e-3)
        kw = dict(sched=(rs.sched, rs.omega), s_base=1, nsweep=len(omegas))
        kw_host = kw
    else:
        cheb = [s > 0 for s in range(len(omegas))] if cheb is None else list(cheb)
        kw = dict(omegas=list(omegas), chebyshev=cheb)
        kw_host = kw
    geo_full = {"w": w, "h": h_total, "halo": 0, "n_up": 0}
    zo, zpo = (torch.zeros(1, ld, device=device) for _ in range(2))
    K.reg_sweeps_tiled(n, u, v, z0, zm1, zo, zpo, gamma, mask, Nf, geo_full, **kw_host)
    # the strip's own arrays and its neighbours' rows
    h = r1 - r0
    N = h * w
    lds = N + 16

    def rows_of(a, ra, rb):
        return a[..., ra * w:rb * w]
    us = torch.zeros(n, lds, device=device)
    vs = torch.zeros(n, lds, device=device)
    us[:, :N] = rows_of(u, r0, r1)
    vs[:, :N] = rows_of(v, r0, r1)
    zs = torch.zeros(1, lds, device=device)
    zps = torch.zeros(1, lds, device=device)
    zs[:, :N] = rows_of(z0, r0, r1)
    zps[:, :N] = rows_of(zm1, r0, r1)
    hu = depth if r0 > 0 else 0
    hd = depth if r1 < h_total else 0
    up = dn = None
    if hu:
        up = torch.stack([rows_of(f[j], r0 - hu, r0) for f, j in ((u, j0), (v, j0), (z0, 0), (zm1, 0))]).contiguous()
    if hd:
        dn = torch.stack([rows_of(f[j], r1, r1 + hd) for f, j in ((u, j0), (v, j0), (z0, 0), (zm1, 0))]).contiguous()
    geo = {"w": w, "h": h, "halo": (1 if hu else 0) | (2 if hd else 0), "n_up": w if hu else 0}
    so, spo = (torch.zeros(1, lds, device=device) for _ in range(2))
    halo = (hu, hd, up, dn)
    if split:
        T = K.reg_tile_rows(h)
        a, b = K.reg_boundary_tile_rows(h, depth, hu > 0, hd > 0)
        for tr in ((0, a), (b, T), (a, b)):
            K.reg_sweeps_tiled(n, us, vs, zs, zps, so, spo, gamma, mask, N, geo, halo=halo, tile_rows=tr, **kw)
    else:
        K.reg_sweeps_tiled(n, us, vs, zs, zps, so, spo, gamma, mask, N, geo, halo=halo, **kw)
    return ((so[:, :N].cpu(), spo[:, :N].cpu()), (rows_of(zo, r0, r1).cpu(), rows_of(zpo, r0, r1).cpu()))


def dense_finish(device, h_total=30, w=44, ranks=3, rank=1, n=7, j0=6, out=True, seed=9):
    """reg_finish on a dense strip of a ``ranks``-strip partition (halo rows
    above/below) with the output dump; returns (x_out, mean, unc) on the CPU.
    On the device with w % 4 == 0 this takes the 16-byte path (FINISH4)."""
    from kafka_inferenceengine_amd.parallel import StripPartition
    rng = np.random.default_rng(seed)
    part = StripPartition(np.ones((h_total, w), bool), rank, ranks)
    geo = part.dense_geometry()
    N = part.N
    lay = part.halo_layout()
    cols = N + lay["n_up"] + lay["n_down"]
    ld = N + 12
    mk = lambda r, c, lo=-1.0, hi=1.0: torch.tensor(rng.uniform(lo, hi, size=(r, c)), dtype=torch.float32,
                                                   device=device)
    u, v, xr = mk(n, ld), mk(n, ld, 0.0, 0.2), mk(n, ld)
    z = mk(1, cols)
    a_prec = mk(n * (n + 1) // 2, ld, 0.5, 4.0)
    xo = torch.zeros(n, ld, device=device)
    part_buf = torch.zeros(4096, dtype=torch.float64, device=device)
    mean = torch.zeros(n, N, device=device)
    unc = torch.zeros(n, N, device=device)
    # out="mean": the mean only (the analysis wrote the uncertainty raster)
    K.reg_finish(n, u, v, z, None, xr, xo, 0.8, 1 << j0, N, partials=part_buf, geo=geo,
                 out=(mean, None if out == "mean" else unc, None) if out else None,
                 a_prec=a_prec if out is True else None)
    return xo[:, :N].cpu(), mean.cpu(), unc.cpu(), float(part_buf.sum())


# --------------------------------------------------------------------------
# Per-pixel fault containment (tests/test_gpu_containment.py): one corrupted
# run "A" and its clean twin "B" over the same pixels, and a float64 model of
# the forecast, the analysis and the status byte.
CONTAIN_N = 6 * 64 + 27      # six whole waves and a tail wave of 27 lanes, natural order
CONTAIN_Q = 0.04


def px(wave, lane):
    return 64 * wave + lane


def _tip_dn_bands(prob, dn):
    """prob["raw"] / prob["bands"] of the DN16 encoding for the DN arrays ``dn`` (0: no observation)."""
    raw, bands = [], []
    for d in dn:
        yy = d * 1e-4
        sig = np.maximum(0.05 * yy, 2.5e-3)
        raw.append(dict(dn=np.where(d > 32767, d - 65536, d).astype(np.int16)))
        bands.append((np.where(d > 0, yy, 0.0), np.where(d > 0, 1 / sig ** 2, 0.0)))
    return dict(prob, raw=raw, bands=bands)


def containment_spec(n=7, mask=1 << 6):
    from kafka_inferenceengine_amd.utils.blocks import pack_matrix
    mu, _, Pi = k.tip_prior()
    return {"mode": 1, "m": np.ones(n), "q": np.full(n, CONTAIN_Q), "prop_mask": mask, "reset_mean": mu,
            "reset_cinv": pack_matrix(Pi)}


def containment_problem(n_train, seed=17, spatial=False):
    """The JRC-TIP state of ``tip_problem(dn16=True)`` under the fused LAI
    forecast (tests/test_gpu_line.py), CONTAIN_N pixels; wave w is pixels
    64 w .. 64 w + 63.  Returns runs ``A`` (corrupted), ``B`` (its clean twin)
    and ``M`` (A with the two pixels whose forecast mean is not finite replaced
    by healthy unobserved ones, which contribute exactly 0 to the norm), each a
    dict(prob, xa [N, 7], pa [N, 7, 7]); ``corrupt``: the pixels whose inputs
    differ between A and B and are read; ``table``: the line table's range of
    the propagated parameter.

    wave 0  observed, clean
    wave 1  observed; lane 3 x_a[6] = NaN, lane 9 p_a = -I, lane 17 p_a[6, 6] =
            NaN, lane 33 x_a[6] = +inf, lane 40 both DN = 0, lane 63 x_a[2] =
            NaN (the forecast does not read it: healthy)
    wave 2  no lane observed, all healthy (the unobserved-wave shortcut)
    wave 3  no lane observed, lane 35 p_a = -I (the shortcut declined)
    wave 4  observed, lanes 5 and 44 finite outside the line table (A and B)
    wave 5  lanes 0-31 observed inside the table, 32-63 unobserved, lanes 37 and
            58 of those outside the table (A and B)
    wave 6  27 lanes, observed; lane 26 (which the tail lanes repeat) p_a = -I

    ``spatial``: seven whole waves (the rows of a raster 64 wide) and of A's
    corruptions only lanes 9 and 17 of wave 1."""
    from kafka_inferenceengine_amd.models.gp import line_table
    N, n = (7 * 64 if spatial else CONTAIN_N), 7
    prob = tip_problem(N=N, seed=seed, n_train=n_train, dn16=True, mask_frac=0.0)
    rng = np.random.default_rng(seed + 1)
    mu = k.tip_prior()[0]
    pa = spd_blocks(rng, N, n, 5.0) * 0.2 + prob["Pf"]
    xa = prob["x"].astype(np.float32).astype(np.float64)
    dn = [np.where(r["dn"] < 0, r["dn"].astype(np.int32) + 65536, r["dn"]).astype(np.int32) for r in prob["raw"]]
    assert all((d > 0).all() for d in dn)
    special = [px(1, l) for l in (3, 9, 17, 33, 40, 63)] + [px(3, 35), px(4, 5), px(4, 44), px(6, 26)]
    # observed waves: one band of every fifth ordinary pixel is missing
    drop = rng.random(N) < 0.2
    drop[special] = False
    which = rng.integers(0, 2, N)
    for b in range(2):
        dn[b][drop & (which == b)] = 0
    dark = np.zeros(N, bool)
    dark[px(2, 0):px(4, 0)] = True
    dark[px(5, 32):px(6, 0)] = True
    for b in range(2):
        dn[b][dark] = 0
    tab = line_table(prob["specs"], np.asarray(mu, dtype=np.float32).astype(np.float64), 6)
    assert tab is not None
    t_lo, t_hi = tab[1], tab[1] + tab[3] / tab[2]
    for p, v in ((px(4, 5), t_hi + 0.25), (px(4, 44), t_lo - 0.25), (px(5, 37), t_hi + 0.25),
                 (px(5, 58), t_lo - 0.25)):
        xa[p, 6] = np.float32(v)
    inside = (xa[:, 6] >= t_lo) & (xa[:, 6] <= t_hi)
    assert inside[px(5, 0):px(5, 32)].all() and inside[px(1, 0):px(2, 0)].all()
    B = dict(prob=_tip_dn_bands(prob, dn), xa=xa, pa=pa)
    xa_a, pa_a, dn_a = xa.copy(), pa.copy(), [d.copy() for d in dn]
    corrupt = np.zeros(N, bool)
    pa_a[px(1, 9)] = -np.eye(n)
    pa_a[px(1, 17), 6, 6] = np.nan
    corrupt[[px(1, 9), px(1, 17)]] = True
    if not spatial:
        xa_a[px(1, 3), 6] = np.nan
        xa_a[px(1, 33), 6] = np.inf
        xa_a[px(1, 63), 2] = np.nan
        for p in (px(3, 35), px(6, 26)):
            pa_a[p] = -np.eye(n)
        for b in range(2):
            dn_a[b][px(1, 40)] = 0
        corrupt[[px(1, 3), px(1, 33), px(1, 40), px(3, 35), px(6, 26)]] = True
    A = dict(prob=_tip_dn_bands(prob, dn_a), xa=xa_a, pa=pa_a)
    xa_m, dn_m = xa_a.copy(), [d.copy() for d in dn_a]
    for p in (px(1, 3), px(1, 33)):
        xa_m[p] = xa[p]
        for b in range(2):
            dn_m[b][p] = 0
    M = dict(prob=_tip_dn_bands(prob, dn_m), xa=xa_m, pa=pa_a)
    # B with one NaN state in the unobserved wave 2: its only reason to decline the shortcut
    xa_c = xa.copy()
    xa_c[px(2, 20), 6] = np.nan
    C = dict(prob=B["prob"], xa=xa_c, pa=pa)
    return dict(A=A, B=B, M=M, C=C, corrupt=corrupt, table=(t_lo, t_hi), N=N, n=n)


def chol_model(A, b):
    """float64 model of the kernels' factor-and-solve (kf_core.h chol_packed,
    chol_solve): a pivot that is not positive and finite fails the SPD test,
    and one that is not positive is replaced by 1.  Returns (spd [N], x [N, n])."""
    N, n, _ = A.shape
    U = np.zeros_like(A)
    spd = np.ones(N, bool)
    with np.errstate(all="ignore"):
        for j in range(n):
            s = A[:, j, j] - (U[:, :j, j] ** 2).sum(1)
            spd &= (s > 0) & np.isfinite(s)
            d = np.sqrt(np.where(s > 0, s, 1.0))
            U[:, j, j] = d
            for i in range(j + 1, n):
                U[:, j, i] = (A[:, j, i] - (U[:, :j, j] * U[:, :j, i]).sum(1)) / d
        z = np.zeros_like(b)
        for i in range(n):
            z[:, i] = (b[:, i] - (U[:, :i, i] * z[:, :i]).sum(1)) / U[:, i, i]
        x = np.zeros_like(b)
        for i in reversed(range(n)):
            x[:, i] = (z[:, i] - (U[:, i, i + 1:] * x[:, i + 1:]).sum(1)) / U[:, i, i]
    return spd, x


def info_model(x0, xf, Pf, evals, dom=None, reg_gd=None, reg_j=6, prior_product=True):
    """float64 model of the information-form analysis of every pixel and of
    the status byte it must carry.  ``evals``: per band (H0 [N], h [N, n], y,
    w) at the linearisation point x0.

    ST_BAD_OP         a used band whose value or Jacobian is not finite
    ST_NO_OBS         no band left
    ST_OUT_OF_DOMAIN  x0 outside the box ``dom`` (BandTable.dom)
    ST_NONSPD         the Cholesky factorisation of the forecast precision or of
                      the analysis precision fails
    ST_NONFINITE      the solution is not finite
    ST_FALLBACK       either of the last two: the pixel keeps the forecast

    ``reg_gd`` [N]: gamma * degree on the regularised parameter's diagonal (the
    spatial twin, which solves the full form b = r + A x0).  ``prior_product``:
    the prior part of the right-hand side is a product with P_f^-1, so a NaN in
    it reaches the solution (the host runner's full form P_f^-1 x_f); False: at
    the forecast the correction form's P_f^-1 (x_f - x0) is written as the 0 it
    is (the matrix-core kernels' first iteration).  Returns the status, the fallback
    mask, the analysis (x, A) by ``analysis_blocks`` on the pixels that keep it
    (the forecast elsewhere) and the norm sum |x - x0|^2 over them."""
    from kafka_inferenceengine_amd.inference import analysis_blocks
    N, n = xf.shape
    st = np.zeros(N, np.uint8)
    with np.errstate(all="ignore"):
        Aa = Pf.copy()
        r = np.einsum("nij,nj->ni", Pf, xf - x0) if prior_product else np.zeros((N, n))
        nobs = np.zeros(N, int)
        used = []
        for H, h, y, w in evals:
            use = w > 0
            ok = np.isfinite(H) & np.isfinite(h).all(1)
            st[use & ~ok] |= K.ST_BAD_OP
            u = use & ok
            nobs += u
            hu, wu, Hu = np.where(u[:, None], h, 0.0), np.where(u, w, 0.0), np.where(u, H, 0.0)
            Aa += wu[:, None, None] * hu[:, :, None] * hu[:, None, :]
            r += (wu * (y - Hu))[:, None] * hu
            used.append((Hu, hu, y, wu))
        st[nobs == 0] |= K.ST_NO_OBS
        if dom is not None:
            lo, hi = (np.asarray(d[:n], dtype=np.float32).astype(np.float64) for d in dom)
            st[~((x0 >= lo) & (x0 <= hi)).all(1)] |= K.ST_OUT_OF_DOMAIN
        spd_f, _ = chol_model(Pf, np.zeros((N, n)))
        if reg_gd is None:
            spd, dx = chol_model(Aa, r)
            sol = x0 + dx
        else:
            r = r + np.einsum("nij,nj->ni", Aa, x0)
            Aa[:, reg_j, reg_j] += reg_gd
            spd, sol = chol_model(Aa, r)
        spd &= spd_f
        fin = np.isfinite(sol).all(1)
    st[~spd] |= K.ST_NONSPD
    st[~fin] |= K.ST_NONFINITE
    fb = ~spd | ~fin
    st[fb] |= K.ST_FALLBACK
    x, A = xf.copy(), Pf.copy()
    keep = ~fb
    xr, Ar = analysis_blocks(x0[keep], xf[keep], Pf[keep], [tuple(a[keep] for a in bd) for bd in used])
    norm = float(((xr - x0[keep]) ** 2).sum())
    if reg_gd is not None:
        # the regulariser's prepare: u = A_reg^-1 b with the unregularised b = A x_a
        b = np.einsum("nij,nj->ni", Ar, xr)
        Ar[:, reg_j, reg_j] += reg_gd[keep]
        xr = np.linalg.solve(Ar, b[..., None])[..., 0]
    x[keep], A[keep] = xr, Ar
    return dict(xf=xf, Pf=Pf, x=x, A=A, status=st, fallback=fb, observed=nobs > 0, norm=norm)


def containment_model(run, dom=None, reg_gd=None, prior_product=False):
    """``info_model`` of one launch of a containment run linearised at its
    fused forecast: the forecast from the reference-API propagator
    (inference/kf_tools.py) over the float32 inputs, the bands from the
    emulators' ``predict``."""
    from kafka_inferenceengine_amd.inference import kf_tools as T
    from kafka_inferenceengine_amd.utils.blocks import sparse_to_blocks
    prob, N, n = run["prob"], run["prob"]["N"], 7
    xa32 = run["xa"].astype(np.float32).astype(np.float64)
    da = np.einsum("nii->ni", run["pa"]).astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        xf, _, Pr = T.propagate_information_filter_LAI(xa32.ravel(), None, da.ravel(), None,
                                                       np.full(N * n, CONTAIN_Q))
        xf = xf.reshape(N, n).astype(np.float32).astype(np.float64)
        Pf = sparse_to_blocks(Pr, n, check=False).astype(np.float64)
        evals = []
        for b, (y, w) in enumerate(prob["bands"]):
            mp = k.TIP_BAND_MAPPER[b]
            H, dH = prob["ems"][b].predict(xf[:, mp])
            h = np.zeros((N, n))
            h[:, mp] = dH
            evals.append((H, h, y, w))
    m = info_model(xf, xf, Pf, evals, dom, reg_gd, 6, prior_product)
    m["H"] = [e[0] for e in evals]
    return m


def containment_launch(run, device, variant=None, line=None, reg=None):
    """One information-form launch of ``run`` linearised at the fused forecast
    with every output the kernel can write; returns CPU arrays."""
    prob = run["prob"]
    n, N = prob["n"], prob["N"]
    nt = n * (n + 1) // 2
    h0 = [torch.zeros(N, dtype=torch.float32, device=device) for _ in range(2)]
    tab = table(prob, device, h0_outs=h0)
    xo = torch.zeros((n, N), device=device)
    ao = torch.zeros((nt, N), device=device)
    st = torch.zeros(N, dtype=torch.uint8, device=device)
    unc = torch.zeros((n, N), device=device)
    h = K.prop_args(n, containment_spec(n), soa(run["xa"], device), packed(run["pa"], device), fused=True)
    K.STRUCT_LAUNCHES.update(tip=0, dense=0)
    res = dict(dom=tab.dom)
    if reg is None:
        mean = torch.zeros((n, N), device=device)
        part = K.partials_buffer(N, device)
        K.analysis(n, tab, None, None, None, xo, ao, None, st, part, prop=h, out=(mean, unc, None), variant=variant,
                   line=line)
        res.update(mean=mean.cpu().numpy(), norm=float(K.reduce_partials(part).cpu()))
    else:
        v = torch.full((n, N), 7.0, device=device)
        K.analysis(n, tab, None, None, None, xo, ao, None, st, None, prop=h, out=(None, unc, None), variant=variant,
                   line=line, reg=dict(reg, v_out=v, nbr=None))
        res.update(v=v.cpu().numpy())
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    res.update(x=xo.cpu().numpy(), a=ao.cpu().numpy(), status=st.cpu().numpy(), unc=unc.cpu().numpy(),
               h0=[t.cpu().numpy() for t in h0], launches=dict(K.STRUCT_LAUNCHES))
    return res


# --------------------------------------------------------------------------
# Auxiliary kernels at every compiled state size (tests/test_gpu_aux.py):
# inputs rounded to float32 first, a float64 NumPy model over exactly those
# values, operands whose leading dimension exceeds N with a sentinel in the
# padding columns.
AUX_NP = (1, 2, 3, 4, 7, 10)
AUX_N = (1, 63, 64, 65, 257 + 256)     # below a wave, around one, two workgroups
AUX_PAD = (5, 64)
SENTINEL = 12345.0


def aux_shape(i):
    """(N, pad) of the i-th case of a kernel: every N and both pads come up."""
    return AUX_N[i % len(AUX_N)], AUX_PAD[i % len(AUX_PAD)]


def f32(a):
    """``a`` rounded to float32, as float64."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def sym32(blocks):
    """[N, n, n] symmetric blocks as the kernels read them: the packed upper
    triangle rounded to float32."""
    from kafka_inferenceengine_amd.utils.blocks import unpack_blocks
    return unpack_blocks(f32(pack_blocks(blocks)), blocks.shape[-1])


def padded(rows, ld, device, fill=SENTINEL, dtype=torch.float32):
    """[R, N] array -> [R, ld] tensor on ``device``, columns N.. hold ``fill``."""
    rows = np.atleast_2d(np.asarray(rows))
    t = torch.full((rows.shape[0], ld), fill, dtype=dtype)
    t[:, :rows.shape[1]] = torch.from_numpy(np.ascontiguousarray(rows)).to(dtype)
    return t.to(device)


def sentinel(rows, ld, device, fill=SENTINEL, dtype=torch.float32):
    return torch.full((rows, ld), fill, dtype=dtype, device=device)


PROP_BLENDS = ("off", "on", "quirk")


def propagate_case(n, N, mode, blend="off", seed=0):
    """Inputs of one propagate launch with per-pixel trajectory uncertainty
    (and, with ``blend``, per-pixel prior mean and precision), and the float64
    model of its result over the formulas of inference/kf_tools.py:

    mode 0  reset:       x_f = reset mean, P_f^-1 = reset precision
    mode 1  partial:     as 0, but x_f[j] = m_j x_a[j] and (P_f^-1)_jj =
                         1 / (1 / A_jj + q_j) for the propagated j
    mode 2  approximate: x_f = m x_a, P_f^-1 = diag(d / (1 + d q)), d = diag A
    mode 3  exact:       x_f = m x_a, P_f^-1 = (A^-1 + Q)^-1
    mode 4  standard:    x_f = m x_a, P_f = A + Q   (A a covariance)
    mode 5  identity:    x_f = m x_a, P unchanged
    blend   the Gaussian product with the prior (mu, C^-1): P + C^-1 and its
            solve of P x_f + C^-1 mu ("on") or P mu + C^-1 x_f ("quirk")

    The propagated parameters are the lowest and the highest.  The constant
    fields of ``spec`` that the per-pixel operands replace hold values that
    would be visibly wrong if read.  Every matrix the kernel factorises is SPD
    (a diagonally dominant reset precision keeps it so under the diagonal
    replacement of mode 1)."""
    from kafka_inferenceengine_amd.utils.blocks import pack_matrix, unpack_matrix
    rng = np.random.default_rng([seed, n, N, mode, PROP_BLENDS.index(blend)])
    A = sym32(spd_blocks(rng, N, n, 5.0))
    xa = f32(rng.normal(size=(N, n)))
    m = f32(rng.uniform(0.9, 1.1, n))
    q = f32(rng.uniform(0.01, 0.2, (N, n)))
    mask = 1 | (1 << (n - 1))
    prop = np.array([(mask >> j) & 1 for j in range(n)], bool)
    mu0 = f32(rng.normal(size=n))
    R = rng.uniform(-0.15, 0.15, (n, n))
    R = 0.5 * (R + R.T)
    np.fill_diagonal(R, 0.0)
    R += np.diag(2.0 + np.abs(R).sum(1))
    R = unpack_matrix(f32(pack_matrix(R)), n)
    mu = f32(mu0[None] + 0.3 * rng.normal(size=(N, n)))
    Ci = sym32(0.5 * spd_blocks(rng, N, n, 3.0))
    d = np.einsum("nii->ni", A)
    mx = m[None] * xa
    if mode == 0:
        xf, P = np.tile(mu0, (N, 1)), np.tile(R, (N, 1, 1))
    elif mode == 1:
        xf, P = np.where(prop[None], mx, mu0[None]), np.tile(R, (N, 1, 1))
        for j in np.nonzero(prop)[0]:
            P[:, j, j] = 1.0 / (1.0 / d[:, j] + q[:, j])
    elif mode == 2:
        xf, P = mx, np.zeros((N, n, n))
        P[:, np.arange(n), np.arange(n)] = d / (1.0 + d * q)
    elif mode == 3:
        Q = np.zeros((N, n, n))
        Q[:, np.arange(n), np.arange(n)] = q
        xf, P = mx, np.linalg.inv(np.linalg.inv(A) + Q)
    elif mode == 4:
        xf, P = mx, A.copy()
        P[:, np.arange(n), np.arange(n)] += q
    else:
        xf, P = mx, A.copy()
    if blend != "off":
        if blend == "quirk":
            b = np.einsum("nij,nj->ni", P, mu) + np.einsum("nij,nj->ni", Ci, xf)
        else:
            b = np.einsum("nij,nj->ni", P, xf) + np.einsum("nij,nj->ni", Ci, mu)
        P = P + Ci
        xf = np.linalg.solve(P, b[..., None])[..., 0]
    assert np.linalg.eigvalsh(A).min() > 0 and np.linalg.eigvalsh(P).min() > 0
    spec = {"mode": mode, "m": m, "q": np.full(n, 50.0), "prop_mask": mask, "reset_mean": mu0,
            "reset_cinv": pack_matrix(R), "blend": blend != "off", "quirk_blend": blend == "quirk",
            "blend_mean": np.full(n, 1e3), "blend_cinv": pack_matrix(100.0 * np.eye(n))}
    return dict(n=n, N=N, mode=mode, blend=blend, spec=spec, xa=xa, A=A, q=q, mu=mu, Ci=Ci, xf=xf, P=P)


def propagate_launch(c, device, pad, A=None, Ci=None, status=False):
    """One launch of ``propagate_case`` ``c`` with ld = N + pad and sentinel-filled
    outputs (``A`` / ``Ci`` replace the case's precision / prior precision);
    returns the CPU tensors (x_f, p_f, status or None), all [*, ld]."""
    n, N = c["n"], c["N"]
    ld = N + pad
    nt = n * (n + 1) // 2
    xf, pf = sentinel(n, ld, device), sentinel(nt, ld, device)
    st = torch.zeros(ld, dtype=torch.uint8, device=device) if status else None
    if st is not None:
        st[N:] = 0xA5
    bl = c["blend"] != "off"
    K.propagate(n, c["spec"], padded(c["xa"].T, ld, device),
                padded(pack_blocks(c["A"] if A is None else A), ld, device), xf, pf, N=N, status=st,
                q_pix=padded(c["q"].T, ld, device),
                blend_mean_pix=padded(c["mu"].T, ld, device) if bl else None,
                blend_cinv_pix=padded(pack_blocks(c["Ci"] if Ci is None else Ci), ld, device) if bl else None)
    return xf.cpu(), pf.cpu(), None if st is None else st.cpu()


def invert_case(n, N, seed=0):
    """SPD blocks and their float64 inverses; ``bad``: about a tenth of the
    pixels (always the last), whose last diagonal entry changes sign in the
    ``B_bad`` copy (not positive definite: the last pivot fails)."""
    rng = np.random.default_rng([seed, n, N])
    B = sym32(spd_blocks(rng, N, n))
    bad = rng.random(N) < 0.1
    bad[N - 1] = True
    B_bad = B.copy()
    B_bad[bad, n - 1, n - 1] *= -1.0
    return dict(n=n, N=N, B=B, inv=np.linalg.inv(B), bad=bad, B_bad=B_bad)


HESSIAN_LAYOUTS = ("tip", "prosail", 2, 3, 4)


def hessian_case(layout, N, seed=0):
    """GP bands for the K6 Hessian correction and its float64 reference
    (``emulator.predict`` / ``emulator.hessian``): "tip" two 4-input bands of
    the 7-parameter state, "prosail" three full-state bands of the
    10-parameter state, 2 / 3 / 4 two full-state bands of a small fitted
    emulator.  A fifth of the pixels is masked (w = 0 in every band); ``a0`` is
    the packed matrix the correction is subtracted from, ``corr`` the
    correction, ``ref`` = a0 - corr (unpacked)."""
    from kafka_inferenceengine_amd.models.gp import GaussianProcessEmulator
    from kafka_inferenceengine_amd.utils.blocks import unpack_blocks
    rng = np.random.default_rng([seed, N, HESSIAN_LAYOUTS.index(layout)])
    if layout == "tip":
        n, ems, maps = 7, k.make_tip_emulators(n_train=64, seed=seed), [list(m) for m in k.TIP_BAND_MAPPER[:2]]
        mu, P, _ = k.tip_prior()
        x = mu[None, :] + rng.normal(size=(N, 7)) * np.sqrt(np.diag(P)) * 0.3
        x[:, 6] = np.clip(x[:, 6], 0.05, 0.95)
    elif layout == "prosail":
        n, ems = 10, k.make_prosail_emulators(n_bands=3, n_train=40, seed=seed)
        maps = [list(range(10))] * 3
        lo = np.min([em.inputs.min(0) for em in ems], 0)
        hi = np.max([em.inputs.max(0) for em in ems], 0)
        x = lo + (hi - lo) * (0.2 + 0.6 * rng.random((N, 10)))
    else:
        n = int(layout)
        v = rng.normal(size=(2, n))
        ems = [GaussianProcessEmulator.synthetic(lambda X, b=b: 0.4 + 0.2 * np.sin(X @ v[b]), np.zeros(n), np.ones(n),
                                                 n_train=30, seed=seed + b) for b in range(2)]
        maps = [list(range(n))] * 2
        x = rng.uniform(0.1, 0.9, (N, n))
    x = f32(x)
    masked = rng.random(N) < 0.2
    masked[0] = False
    if N > 1:
        masked[N // 2] = True
    obs, corr = [], np.zeros((N, n, n))
    for em, mp in zip(ems, maps):
        f, _ = em.predict(x[:, mp])
        y = f32(f + 0.01 * rng.normal(size=N))
        w = f32(np.where(masked, 0.0, 1.0 / 0.02 ** 2))
        obs.append((y, w))
        corr[np.ix_(np.arange(N), mp, mp)] += (w * (y - f))[:, None, None] * em.hessian(x[:, mp])
    nt = n * (n + 1) // 2
    a0 = f32(rng.normal(size=(nt, N)))
    specs = [k.gp_spec(em, mp) for em, mp in zip(ems, maps)]
    return dict(n=n, N=N, x=x, obs=obs, specs=specs, masked=masked, a0=a0, corr=corr,
                ref=unpack_blocks(a0, n) - corr)


def hessian_launch(c, device, pad):
    """K6 on ``hessian_case`` ``c`` in place on a copy of a0 with ld = N + pad;
    returns the CPU tensor [nt, ld]."""
    n, N = c["n"], c["N"]
    ld = N + pad
    db = [DeviceBand(K.OBS_F32, y=torch.from_numpy(y.astype(np.float32)).to(device),
                     w=torch.from_numpy(w.astype(np.float32)).to(device)) for y, w in c["obs"]]
    tab = build_table(c["specs"], db, n, RecordCache(), device)
    a = padded(c["a0"], ld, device)
    K.hessian(n, tab, padded(c["x"].T, ld, device), a, N=N)
    return a.cpu()


def unpack_case(n, N, seed=0):
    """State, SPD precision and a sorted index map into a raster of 2 N + 7
    cells, of which the last is named by no pixel."""
    rng = np.random.default_rng([seed, n, N])
    plane = 2 * N + 7
    return dict(n=n, N=N, x=f32(rng.normal(size=(N, n))), A=sym32(spd_blocks(rng, N, n)), plane=plane,
                idx=np.sort(rng.choice(plane - 1, N, replace=False)).astype(np.int64))


# K7: (M, D) of the LUT; 4096 x 4 floats are exactly 64 KiB, 5000 x 10 the
# reference's default LUT over a full PROSAIL state
LUT_SIZES = ((1, 3), (50, 3), (4096, 4), (4097, 4), (5000, 4), (5000, 7), (5000, 10))
LUT_N = (1, 63, 65, 4096 + 37)
_LUT_CASES: dict = {}


def lut_case(M, D, seed=0):
    """4133 multivariate-normal points and an M-row LUT drawn from their mean
    and covariance (as run_emulator draws it), both rounded to float32, with
    the float64 nearest row of every point over those values: ``near`` its
    index, ``dmin`` its squared distance.  Built once per (M, D)."""
    key = (M, D, seed)
    if key not in _LUT_CASES:
        rng = np.random.default_rng([seed, M, D])
        G = rng.normal(size=(D, D))
        pts = f32(rng.multivariate_normal(np.full(D, 0.5), 0.01 * (G @ G.T / D + 0.5 * np.eye(D)), LUT_N[-1]))
        lut = f32(rng.multivariate_normal(pts.mean(0), np.cov(pts, rowvar=False), M))
        near = np.empty(len(pts), np.int64)
        l2 = (lut * lut).sum(1)
        for s in range(0, len(pts), 512):
            near[s:s + 512] = (l2[None, :] - 2.0 * pts[s:s + 512] @ lut.T).argmin(1)
        _LUT_CASES[key] = dict(M=M, D=D, pts=pts, lut=lut, near=near, dmin=lut_dist(lut, pts, near))
    return _LUT_CASES[key]


def lut_dist(lut, pts, idx):
    """float64 squared distance of every point to its LUT row ``idx``."""
    t = lut[np.asarray(idx, dtype=np.int64)] - pts
    return (t * t).sum(1)


def lut_launch(lut, pts, N, device):
    """K7 over the first N points given as [D, ld], ld = N + 11; the padding
    holds points far from the LUT and the output a sentinel past N.  Returns
    the CPU int32 tensor [ld]."""
    ld = N + 11
    out = torch.full((ld,), -7, dtype=torch.int32, device=device)
    x = padded(np.asarray(pts)[:N].T, ld, device, fill=1e6)
    K.lut_nearest(torch.from_numpy(np.asarray(lut, dtype=np.float32)).to(device), x, out=out, N=N)
    return out.cpu()


# --------------------------------------------------------------------------
# The non-GP analysis and gain kernels (tests/test_nongp_kernels.py): linear,
# precomputed and mixed band tables in every observation encoding, built from
# raw bits, with a float64 model of decode_obs, of the operators and (through
# info_model / gain_blocks) of the analysis and its status byte.
ENCODINGS = (K.OBS_DN16, K.OBS_F32, K.OBS_BF16, K.OBS_BF16Y)
ENC_NAME = {K.OBS_DN16: "dn16", K.OBS_F32: "f32", K.OBS_BF16: "bf16", K.OBS_BF16Y: "bf16y"}
# DN 65535 is a reflectance of 0.655: the clean observations (<= 0.6) use the whole uint16 range
NONGP_SCALE, NONGP_REL, NONGP_FLOOR = 1e-5, 0.05, 2.5e-3
STATUS_FILL = 0xA5


def bf16_bits(a):
    """float32 values -> bf16 bit patterns (uint16), round to nearest even; Inf and NaN keep their class."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(a, dtype=np.float32))
    return np.where(nan, np.uint16(0x7FC0), r).astype(np.uint16)


def bf16_value(bits):
    """bf16 bit patterns (uint16) -> their values as float64: the bits shifted left by 16, read as float32."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def decode_model(enc, raw, scale=NONGP_SCALE, rel_unc=NONGP_REL, unc_floor=NONGP_FLOOR):
    """float64 model of kf_core.h decode_obs from the raw bits of one band:
    ``raw["dn"]`` uint16 digital numbers, or ``raw["y"]`` / ``raw["w"]`` float32
    values (OBS_F32) or bf16 bit patterns (OBS_BF16; OBS_BF16Y has y only), and
    ``raw["mask"]`` uint8 or None.  Returns (y, w), both 0 where the band has no
    observation:

    DN16   y = f32(DN scale); sigma = max(rel_unc y, floor); kept where DN > 0
           and sigma > 0 with w = 1 / sigma^2 (y is kept wherever DN > 0)
    F32    kept where the mask (if any) is set, w > 0, w and y finite
    BF16   as F32 on the values of the bit patterns
    BF16Y  sigma = max(rel_unc |y|, floor); kept where the mask is set, y is
           finite and sigma > 0, w = 1 / sigma^2

    The weight 1 / sigma^2 is taken in float64 from the float32-rounded y and
    the float32-rounded scalars."""
    s, r, fl = (float(np.float32(v)) for v in (scale, rel_unc, unc_floor))
    with np.errstate(all="ignore"):
        if enc == K.OBS_DN16:
            dn = np.asarray(raw["dn"], dtype=np.uint16).astype(np.float64)
            y = f32(dn * s)
            sig = np.maximum(r * y, fl)
            ok = (dn > 0) & (sig > 0)
            return np.where(dn > 0, y, 0.0), np.where(ok, 1.0 / np.where(ok, sig * sig, 1.0), 0.0)
        m = np.ones(len(raw["y"]), bool) if raw.get("mask") is None else np.asarray(raw["mask"]) != 0
        if enc == K.OBS_BF16Y:
            y = bf16_value(raw["y"])
            sig = np.maximum(r * np.abs(y), fl)
            ok = m & np.isfinite(y) & (sig > 0)
            return np.where(ok, y, 0.0), np.where(ok, 1.0 / np.where(ok, sig * sig, 1.0), 0.0)
        if enc == K.OBS_BF16:
            y, w = bf16_value(raw["y"]), bf16_value(raw["w"])
        else:
            y, w = (np.asarray(raw[key], dtype=np.float32).astype(np.float64) for key in ("y", "w"))
        ok = m & (w > 0) & np.isfinite(w) & np.isfinite(y)
        return np.where(ok, y, 0.0), np.where(ok, w, 0.0)


# decode edges, planted in every band at pixel 1 + i and in band i % nb alone at
# pixel 20 + i (the pixel is then still observed by the other bands).  Each
# entry replaces fields of the encoded observation: dn, y, w (values), mask.
DECODE_EDGES = {
    K.OBS_DN16: (dict(dn=0), dict(dn=1), dict(dn=32768), dict(dn=40000), dict(dn=65535)),
    K.OBS_F32: (dict(w=0.0), dict(w=-4.0), dict(w=np.inf), dict(w=np.nan), dict(w=-np.inf), dict(y=np.nan),
                dict(y=np.inf), dict(y=-np.inf), dict(mask=0), dict(w=2.0 ** 20)),
    K.OBS_BF16Y: (dict(y=np.nan), dict(y=np.inf), dict(y=-np.inf), dict(y=-0.3125), dict(y=0.0), dict(mask=0)),
}
DECODE_EDGES[K.OBS_BF16] = DECODE_EDGES[K.OBS_F32]
EDGE_ALL, EDGE_ONE = 1, 20      # first pixel of the two plant runs
DARK_LANE, LIT_LANE = 40, 41    # of every 64-pixel block: no band observed / every band observed


def encode_band(enc, y, sigma, rng, edges=True, band=0, nb=1, mask_plane=True):
    """One band's raw observation arrays in encoding ``enc`` from clean values
    ``y`` (in (0, 0.65)) with standard deviations ``sigma``: a quarter of the pixels
    dropped at random through the encoding's own nodata value, the decode edges
    planted, lanes DARK_LANE / LIT_LANE of every 64-pixel block unobserved /
    observed (a block of one pixel, the tail of N = 65 or 513, is observed).
    Returns the raw dict of ``decode_model``."""
    N = len(y)
    drop = rng.random(N) < 0.25
    lane, blk = np.arange(N) % 64, np.arange(N) // 64
    single = np.bincount(blk)[blk] == 1
    drop[(lane == LIT_LANE) | single] = False
    drop[(lane == DARK_LANE) & ~single] = True
    f = dict(dn=np.clip(np.round(y / NONGP_SCALE), 1, 65535), y=np.array(y, dtype=np.float64),
             w=1.0 / np.asarray(sigma, dtype=np.float64) ** 2, mask=np.ones(N))
    # the nodata value of the encoding; with a mask plane every other dropped pixel goes through it alone
    via_mask = drop & (np.arange(N) % 2 == 0) & (enc != K.OBS_DN16) & mask_plane
    f["mask"][via_mask] = 0
    hard = drop & ~via_mask
    f["dn"][hard] = 0
    if enc == K.OBS_BF16Y:
        f["y"][hard] = np.nan
    else:
        f["w"][hard] = 0.0
    if edges:
        for i, e in enumerate(DECODE_EDGES[enc]):
            for p in (EDGE_ALL + i,) + ((EDGE_ONE + i,) if band == i % nb else ()):
                if p >= N:
                    continue
                # a clean observation, then the edge
                f["dn"][p], f["y"][p], f["w"][p], f["mask"][p] = max(round(y[p] / NONGP_SCALE), 1), y[p], \
                    1.0 / sigma[p] ** 2, 1
                for key, v in e.items():
                    if key == "mask" and not mask_plane:
                        key, v = ("y", np.nan) if enc == K.OBS_BF16Y else ("w", 0.0)
                    f[key][p] = v
    mask = f["mask"].astype(np.uint8) if (mask_plane and enc != K.OBS_DN16) else None
    if enc == K.OBS_DN16:
        return dict(dn=f["dn"].astype(np.uint16), mask=None)
    with np.errstate(all="ignore"):
        y32, w32 = f["y"].astype(np.float32), f["w"].astype(np.float32)
    if enc == K.OBS_F32:
        return dict(y=y32, w=w32, mask=mask)
    if enc == K.OBS_BF16:
        return dict(y=bf16_bits(y32), w=bf16_bits(w32), mask=mask)
    return dict(y=bf16_bits(y32), mask=mask)


def _np_vec(a, ld, device, fill, dtype):
    t = torch.full((ld,), fill, dtype=dtype)
    t[:len(a)] = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    return t.to(device)


def device_band(enc, raw, ld, device, aux=None):
    """``raw`` (encode_band) as a DeviceBand whose vectors are ld long (the
    padding holds values a kernel reading past N would turn into observations)."""
    mask = None if raw.get("mask") is None else _np_vec(raw["mask"], ld, device, 1, torch.uint8)
    kw = dict(scale=NONGP_SCALE, rel_unc=NONGP_REL, unc_floor=NONGP_FLOOR, mask=mask,
              aux=None if aux is None else _np_vec(aux, ld, device, 30.0, torch.float32))
    if enc == K.OBS_DN16:
        return DeviceBand(enc, dn=_np_vec(raw["dn"].view(np.int16), ld, device, 5000, torch.int16), **kw)
    if enc == K.OBS_F32:
        return DeviceBand(enc, y=_np_vec(raw["y"], ld, device, 0.5, torch.float32),
                          w=_np_vec(raw["w"], ld, device, 1e4, torch.float32), **kw)
    one = int(bf16_bits(np.float32([0.5])).view(np.int16)[0])
    y = _np_vec(raw["y"].view(np.int16), ld, device, one, torch.int16)
    if enc == K.OBS_BF16Y:
        return DeviceBand(enc, y=y, **kw)
    return DeviceBand(enc, y=y, w=_np_vec(raw["w"].view(np.int16), ld, device,
                                          int(bf16_bits(np.float32([1e4])).view(np.int16)[0]), torch.int16), **kw)


_NONGP_CASES: dict = {}
_SMALL_GP: dict = {}


def small_gp(n):
    """A 64-point synthetic emulator over all n states (the "small" emulator of test_gpu_launch_plan.py)."""
    from kafka_inferenceengine_amd.models.gp import GaussianProcessEmulator
    if n not in _SMALL_GP:
        _SMALL_GP[n] = GaussianProcessEmulator.synthetic(
            lambda X: 0.3 + 0.2 * np.sin(2 * X[:, 0]) + 0.15 * X[:, 1 % n] * X[:, n - 1], np.zeros(n), np.ones(n),
            64, 5, name="small")
    return _SMALL_GP[n]


def nongp_case(n, N, bands, seed=0, fused=False, bad_op=True):
    """One analysis problem over ``bands`` = ((operator, encoding), ...) with
    operator in "linear", "precomp", "sar", "gp", built once per argument set
    and never changed.  Every input is float32-valued; ``evals`` holds the
    float64 model (H0, h, y, w) of every band at the linearisation point ``x0``
    and ``obs_w`` the decoded weights [nb, N].

    linear   dense positive coefficients over all n states and an offset > 0
    precomp  per-pixel rows pre_h0 [N] / pre_h [n, N]; with ``bad_op`` NaN / Inf
             planted at lanes 45-48 of the first block: 45 pre_h0 of band 0, 46
             one pre_h entry of band 1 (or 0), 47 pre_h0 of every band (the
             pixel then has no usable band), 48 pre_h0 of band 0 at a pixel
             where that band is masked (no flag)
    sar      the water-cloud model on states (0, 1), per-pixel incidence angle
    gp       small_gp(n) over all states

    The forecast precision ``Pf`` is a random SPD block per pixel and ``Pcov``
    its float64 inverse rounded to float32 (the gain form's forecast covariance).

    ``fused``: the forecast is the partial prior reset the kernel computes from
    a previous analysis (``xa``, precision ``pa``; ``spec`` for K.prop_args): the
    last parameter propagated with m = 1, x_f = reset mean elsewhere, P_f^-1 =
    the reset precision with that parameter's diagonal 1 / (1 / pa_jj + q_j), in
    float64 from the float32 inputs; linearised at the forecast (x0 = xf)."""
    from kafka_inferenceengine_amd.models.operators import OP_LINEAR, OP_PRECOMP, OperatorSpec, _sar_device_spec
    from kafka_inferenceengine_amd.utils.blocks import pack_matrix, unpack_matrix
    key = (n, N, tuple(bands), seed, fused, bad_op)
    if key in _NONGP_CASES:
        return _NONGP_CASES[key]
    nb = len(bands)
    rng = np.random.default_rng([seed, n, N] + [("linear", "precomp", "sar", "gp").index(o) * 8 + e for o, e in bands])
    extra = {}
    if fused:
        j, q = n - 1, f32(np.full(n, 0.04))
        mu, xa, pa = f32(rng.uniform(0.25, 0.75, n)), f32(rng.uniform(0.25, 0.75, (N, n))), \
            sym32(spd_blocks(rng, N, n, 10.0))
        R = rng.uniform(-0.15, 0.15, (n, n))
        R = 0.5 * (R + R.T)
        np.fill_diagonal(R, 0.0)
        R += np.diag(2.0 + np.abs(R).sum(1))
        R = unpack_matrix(f32(pack_matrix(R)), n)
        xf, Pf = np.tile(mu, (N, 1)), np.tile(R, (N, 1, 1))
        xf[:, j] = xa[:, j]
        Pf[:, j, j] = 1.0 / (1.0 / pa[:, j, j] + q[j])
        x0 = xf
        extra = dict(xa=xa, pa=pa, spec={"mode": 1, "m": np.ones(n), "q": q, "prop_mask": 1 << j, "reset_mean": mu,
                                         "reset_cinv": pack_matrix(R)})
    else:
        xf = f32(rng.uniform(0.25, 0.75, (N, n)))
        x0 = f32(xf + 0.03 * rng.normal(size=(N, n)))
        Pf = sym32(spd_blocks(rng, N, n, 10.0))
    xt = xf + 0.05 * rng.normal(size=(N, n))
    Pcov = sym32(np.linalg.inv(Pf))
    th = f32(rng.uniform(25, 45, N))
    specs, raws, pre, aux, evals, obs_w = [], [], [], [], [], []
    lane0 = np.arange(N)
    for b, (op, enc) in enumerate(bands):
        p_h0 = p_h = a = None
        if op == "linear":
            c, off = f32(rng.uniform(0.05, 0.3, n) * min(1.0, 2.0 / n)), float(f32(rng.uniform(0.05, 0.2)))
            specs.append(OperatorSpec(OP_LINEAR, list(range(n)), [float(v) for v in c], [], off))
            H0, h = off + x0 @ c, np.tile(c, (N, 1))
            clean = off + xt @ c
        elif op == "precomp":
            p_h0, p_h = f32(rng.uniform(0.1, 0.6, N)), f32(0.3 * rng.normal(size=(N, n)))
            specs.append(OperatorSpec(OP_PRECOMP, list(range(n)), [0.0] * n))
            clean = p_h0 + ((xt - x0) * p_h).sum(1)
            H0, h = p_h0.copy(), p_h.copy()
        elif op == "sar":
            pol = ("VV", "VH")[b % 2]
            specs.append(_sar_device_spec(n, None, None, b % 2))
            H0, g = k.sar_observation_operator(x0[:, :2], th, pol)
            h = np.zeros((N, n))
            h[:, :2] = g
            clean, a = k.sar_observation_operator(xt[:, :2], th, pol)[0], th
        else:
            em = small_gp(n)
            specs.append(k.gp_spec(em, np.arange(n)))
            H0, h = em.predict(x0)
            clean = em.predict(xt)[0]
        sigma = rng.uniform(0.005, 0.02, N)
        clean = np.clip(clean + sigma * rng.normal(size=N), 2e-3, 0.6)
        raw = encode_band(enc, clean, sigma, rng, band=b, nb=nb, mask_plane=not (nb >= 3 and b == nb - 1))
        y, w = decode_model(enc, raw)
        if op == "precomp" and bad_op:
            def at(lane):
                return lane0[lane:lane + 1] if lane < N else lane0[:0]
            if b == 0:
                p_h0[at(45)] = np.nan
                p_h0[at(48)] = np.inf
            if b == min(1, nb - 1):
                p_h[at(46), n - 1] = -np.inf
            p_h0[at(47)] = np.nan
            H0, h = p_h0.copy(), p_h.copy()
        raws.append(raw)
        pre.append(None if p_h0 is None else (p_h0, p_h))
        aux.append(a)
        evals.append((H0, h, y, w))
        obs_w.append(w)
    obs_w = np.array(obs_w)
    if bad_op and N > 48:
        # lanes 45-47 carry the operator faults at observed pixels, lane 48 at a pixel masked in band 0
        for b, (op, enc) in enumerate(bands):
            if op != "precomp":
                continue
            lit = encode_band(enc, np.full(N, 0.4), np.full(N, 0.01), np.random.default_rng(1), edges=False,
                              mask_plane=raws[b].get("mask") is not None)
            for key in raws[b]:
                if raws[b][key] is None:
                    continue
                raws[b][key][45:48] = lit[key][LIT_LANE]
                raws[b][key][48] = lit[key][LIT_LANE if b else DARK_LANE]
            y, w = decode_model(enc, raws[b])
            evals[b] = (evals[b][0], evals[b][1], y, w)
            obs_w[b] = w
    c = dict(n=n, N=N, nb=nb, bands=tuple(bands), specs=specs, raws=raws, pre=pre, aux=aux, x0=x0, xf=xf, Pf=Pf,
             Pcov=Pcov, evals=evals, obs_w=obs_w, **extra)
    _NONGP_CASES[key] = c
    return c


def coverage(c):
    """Every 64-pixel block of the case with more than one pixel holds an observed
    and an unobserved pixel, and a block of one pixel is observed (model weights)."""
    seen = (c["obs_w"] > 0).any(0)
    for s in range(0, c["N"], 64):
        blk = seen[s:s + 64]
        if not (blk.any() and (len(blk) == 1 or not blk.all())):
            return False
    return True


def nongp_table(c, device, pad, h0_out=False, bands=None):
    """The case's band table on ``device`` with ld = N + pad for the observation
    vectors and pre_ld = ld + 3 for the precomputed rows; -> (table, h0 planes
    or None).  ``bands``: the indices of a subset (band chunks)."""
    N, n = c["N"], c["n"]
    ld = N + pad
    idx = list(range(c["nb"])) if bands is None else list(bands)
    db = [device_band(c["bands"][i][1], c["raws"][i], ld, device, c["aux"][i]) for i in idx]
    pre = [None if c["pre"][i] is None else (_np_vec(c["pre"][i][0], ld, device, 0.25, torch.float32),
                                             padded(c["pre"][i][1].T, ld + 3, device, fill=0.25)) for i in idx]
    h0 = [sentinel(1, ld, device)[0] for _ in idx] if h0_out else None
    return build_table([c["specs"][i] for i in idx], db, n, RecordCache(), device, h0, pre), h0


def gain_model(c):
    """float64 model of a gain-form launch of the case: ``gain_blocks`` over the
    bands that are observed and whose operator is finite, and the status byte
    (ST_BAD_OP: an observed band whose value or Jacobian is not finite;
    ST_NO_OBS: no band left).  -> dict(x, P, status, strong): ``strong`` the
    pixels where sum_b w_b h_b^T P_f h_b exceeds 1e2 (the update cancels all but
    1e-2 of the forecast variance along h)."""
    from kafka_inferenceengine_amd.inference import gain_blocks
    N = c["N"]
    st, nobs, used, gain = np.zeros(N, np.uint8), np.zeros(N, int), [], np.zeros(N)
    with np.errstate(all="ignore"):
        for H, h, y, w in c["evals"]:
            use = w > 0
            ok = np.isfinite(H) & np.isfinite(h).all(1)
            st[use & ~ok] |= K.ST_BAD_OP
            u = use & ok
            nobs += u
            hu, wu = np.where(u[:, None], h, 0.0), np.where(u, w, 0.0)
            used.append((np.where(u, H, 0.0), hu, y, wu))
            gain += wu * np.einsum("ni,nij,nj->n", hu, c["Pcov"], hu)
    st[nobs == 0] |= K.ST_NO_OBS
    x, P = gain_blocks(c["x0"], c["xf"], c["Pcov"], used)
    return dict(x=x, P=P, status=st, strong=gain > 1e2)
