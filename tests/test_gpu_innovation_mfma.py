"""``K.innovation(gp="mfma")`` (csrc/kf_gp_mfma.h ``pixel_innovation_mfma``) against the emulators' float64
``predict`` within the bounds of test_innovation.py / test_evidence.py; every launch asserts the kernel it took."""
import numpy as np
import pytest
import torch

import kafka_inferenceengine_amd as k
from kafka_inferenceengine_amd.inference import innovation_blocks
from kafka_inferenceengine_amd.ops import kernels as K

import kernel_cases as C
import test_innovation as TI
from test_evidence import compare
from test_innovation import GROUPS5, NS, SENT, SENT8, near_gate, rejected_of, screened_like, tip_case, z_bound
from test_innovation_mfma import GLOBAL, LDS, gp_table
from test_marginal import blocks_of, pack_rows, spd_blocks

pytestmark = pytest.mark.gpu
_CASES = {}


def gp_case(state, N, kind):
    """JRC-TIP (tip_case) or five PROSAIL bands at hessian_case("prosail")'s x, float64 ``predict``, built once."""
    if (state, N) not in _CASES:
        if state == "tip":
            prob, x32, ob = tip_case(N)
            P, specs = C.sym32(prob["Pf"]), prob["specs"]
            y, w = (np.stack([C.f32(r[key]) for r in prob["raw"]]) for key in ("y", "w"))
        else:
            rng = np.random.default_rng([3, N])
            ems = k.make_prosail_emulators(n_bands=5, n_train=40, seed=0)
            specs = [k.gp_spec(em, range(10)) for em in ems]
            lo, hi = np.min([em.inputs.min(0) for em in ems], 0), np.max([em.inputs.max(0) for em in ems], 0)
            x32 = C.f32(lo + (hi - lo) * (0.2 + 0.6 * rng.random((N, 10))))
            ob = [em.predict(x32) for em in ems]
            P = blocks_of(pack_rows(spd_blocks(10, 1e2, N, 5), N), 10, N)
            s = np.stack([np.einsum("pi,pij,pj->p", dH, np.linalg.inv(P), dH) for _, dH in ob])
            y = C.f32(np.stack([f for f, _ in ob]) + 2.0 * rng.standard_normal((5, N)) * np.sqrt(s + 4e-4))
            w = C.f32(np.where(rng.random((5, N)) < 0.2, 0.0, 2500.0))
        H0, h = np.stack([o[0] for o in ob]), np.stack([o[1] for o in ob])
        _CASES[state, N] = dict(n=x32.shape[1], nb=len(specs), N=N, specs=specs, x=x32, P=P, y=y, w=w, H0=H0, h=h,
                                r_scale=np.abs(H0) + np.abs(y), family=LDS if state == "tip" else GLOBAL)
    g = dict(_CASES[state, N], state=state, kind=kind)
    g["A"] = g["P"] if kind == "precision" else C.sym32(np.linalg.inv(g["P"]))
    g["cov"] = np.linalg.inv(g["A"]) if kind == "precision" else g["A"]
    return g


def launch(g, gp="mfma", joint=False, screened=False, x=None, A=None, **kw):
    n, N, dev = g["n"], g["N"], "cuda"
    tab, obs = gp_table(g["specs"], n, dev, g["y"], g["w"])
    o = dict(z=torch.full((g["nb"], N), SENT, device=dev),
             **{key: torch.full((N,), SENT, device=dev) for key in ("chi2", "d2", "logdet")[:3 if joint else 1]},
             **{key: torch.full((N,), SENT8, dtype=torch.uint8, device=dev) for key in ("nobs", "nrej", "status")})
    scr = [t.to(dev) for t in screened_like(obs)] if screened else None
    K.innovation(n, tab, C.soa(g["x"] if x is None else x, dev), C.packed(g["A"] if A is None else A, dev),
                 kind=g["kind"], screened=scr, gp=gp, **o, **kw)
    plan = K.LAST_INNOVATION_PLAN
    assert (plan["family"], plan["joint"]) == (g["family"] if gp == "mfma" else "pixel_kernel", joint)
    return dict({key: v.cpu().numpy() for key, v in o.items()}, obs=obs, screened=scr and [t.cpu() for t in scr])


def truth(g, **gate):
    """The float64 oracle and the z bound with the GP operator tolerances carried as check_gp does."""
    h, cov = g["h"], g["cov"]
    z64, _, nobs64, rej64 = innovation_blocks(g["A"], g["y"], g["w"], g["H0"], h, kind=g["kind"], **gate)
    counted = ~np.isnan(z64)
    ph = np.abs(np.einsum("pij,bpj->bpi", cov, h)).sum(axis=2)
    bound = z_bound(g["n"], g["A"], np.einsum("bpi,pij,bpj->bp", h, cov, h), np.where(counted, g["w"], 1.0),
                    g["r_scale"], np.nan_to_num(z64), e_r_extra=5e-6, e_s_extra=2.0 * 5e-5 * ph)
    return z64, nobs64, rej64, counted, ph, bound


@pytest.mark.parametrize("joint", [False, True])
@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("state,N,walk", [("tip", N, False) for N in NS] + [
    ("prosail", 65, False), ("prosail", 785, False), ("tip", 785, True), ("prosail", 785, True)])
def test_against_float64_predict(state, N, walk, kind, joint):
    """walk: one workgroup walks all 785 pixels, wave 1 masked in every band (it skips every sum), wave 2 in band 1."""
    g = gp_case(state, N, kind)
    if walk:
        g["w"] = g["w"].copy()
        g["w"][:, 64:128], g["w"][1, 128:192] = 0.0, 0.0
    z64, nobs64, _, counted, ph, bound = truth(g)
    before = K.ext().get_max_blocks()
    K.ext().set_max_blocks(1 if walk else before)
    try:
        for gp in ("valu", "mfma"):
            out = launch(g, gp, joint)
            assert np.array_equal(np.isnan(out["z"]), ~counted)
            err = np.abs(np.where(counted, out["z"] - np.nan_to_num(z64), 0.0))
            print(f"{state} N={N} {kind} joint={joint} walk={walk} {gp}: z max err/bound {np.max(err / bound):.3f}")
    finally:
        K.ext().set_max_blocks(before)
    assert np.all(err <= bound) and (not walk or (not nobs64[64:128].any() and nobs64[128:192].any()))
    assert np.array_equal(out["nobs"], nobs64) and not out["status"].any() and not out["nrej"].any()
    own = np.sum(np.nan_to_num(out["z"].astype(np.float64)) ** 2, axis=0)
    assert np.all(np.abs(out["chi2"] - own) <= (g["nb"] + 1) * TI.U * own)
    if joint:      # test_evidence.check_joint_gp's first-order terms of the operator tolerances
        ex_d, ex_l = np.zeros(N), np.zeros(N)
        for p in np.nonzero(counted.any(axis=0))[0]:
            sel = counted[:, p]
            hp = g["h"][sel, p]
            Si = np.linalg.inv(hp @ g["cov"][p] @ hp.T + np.diag(1.0 / g["w"][sel, p]))
            u = np.abs(Si @ (g["y"][sel, p] - g["H0"][sel, p]))
            dS = 5e-5 * (ph[sel, p][:, None] + ph[sel, p][None, :])
            ex_d[p], ex_l[p] = 2.0 * u.sum() * 5e-6 + u @ dS @ u, np.sum(np.abs(Si) * dS)
        compare(g, out, f"{state} N={N} {kind} walk={walk} mfma", extra_d2=ex_d, extra_ld=ex_l)


@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
@pytest.mark.parametrize("state", ["tip", "prosail"])
def test_containment(state, kind):
    """A non-SPD block and a NaN state in two lanes of wave 1 fail open; every other pixel keeps the clean bits."""
    g = gp_case(state, 200, kind)
    kw = dict(joint=True, screened=True, gate=1.0, scope="band")
    clean = launch(g, **kw)
    x, A = g["x"].copy(), g["A"].copy()
    A[70], x[75, g["n"] - 1] = -np.eye(g["n"]), np.nan
    out = launch(g, x=x, A=A, **kw)
    bad = np.isin(np.arange(200), (70, 75))
    assert np.all(out["status"][bad] == 1) and not out["nrej"][bad].any() and not out["nobs"][bad].any() and \
        all(np.isnan(out[key][..., bad]).all() for key in ("z", "chi2", "d2", "logdet"))
    for key in ("z", "chi2", "nobs", "nrej", "status", "d2", "logdet"):
        assert np.array_equal(out[key][..., ~bad], clean[key][..., ~bad], equal_nan=True), key
    for a, b, o in zip(out["screened"], clean["screened"], out["obs"]):
        assert torch.equal(a[~bad], b[~bad]) and torch.equal(a[bad], o.w.cpu()[bad])


@pytest.mark.parametrize("scope", K.INNOVATION_SCOPES)
@pytest.mark.parametrize("kind", K.MARGINAL_KINDS)
def test_decisions_against_the_oracle(kind, scope):
    """Five PROSAIL bands in two groups, gate 3: rejects and screened planes equal the float64 oracle's off the
    band-pixels within the z bound of the gate: 0.25 % of them (band scope), 0.69 % (group), from the oracle alone."""
    g = gp_case("prosail", 785, kind)
    z64, _, rej64, _, _, bound = truth(g, gate=3.0, scope=scope, groups=GROUPS5)
    near = near_gate(g, z64, bound, 3.0, scope, GROUPS5)
    print(f"prosail {kind} {scope}: rejected {rej64.mean():.3f}, near the gate {near.mean():.5f}")
    assert near.mean() <= 0.01 and 0.02 < rej64.mean() < 0.6
    out = launch(g, screened=True, gate=3.0, scope=scope, groups=GROUPS5)
    rej = rejected_of(g, out)
    assert np.array_equal(rej[~near], rej64[~near]) and np.array_equal(out["nrej"], rej.sum(axis=0))


@pytest.mark.parametrize("form,encoding,scope", [("information", "f32", "group"), ("gain", "dn16", "band")])
def test_engine_option(form, encoding, scope, monkeypatch):
    """test_innovation's two engine checks with every gated run under innovation_gp="mfma"."""
    inner, K.LAST_INNOVATION_PLAN = TI.engine_run, None
    monkeypatch.setattr(TI, "engine_run", lambda *a, **kw: inner(
        *a, **kw, **({"innovation_gp": "mfma"} if kw.get("innovation_gate") else {})))
    TI.check_engine_gated_equals_edited(form, encoding, scope, device="cuda")
    TI.check_engine_patch(form, device="cuda")
    assert K.LAST_INNOVATION_PLAN["family"] == LDS
