"""Transforms from the filter's state space to physical units.

The filter works on transformed parameters (JRC-TIP: ``TeLAI = exp(-LAI / 2)``;
the SAIL state: ``exp(-cab / 100)``, ``exp(-50 cw)``, ``ala / 90`` ...), in
which the emulators are close to linear.  A ``ParameterTransform`` carries one
parameter back: the product rasters (``KafkaOutput(physical=...)``) hold
``T(x_j)`` and the interval ``T(x_j -+ z sigma_j)``, which is the exact
credible interval of a monotone transform of a Gaussian marginal
(``csrc/kf_core.h: pixel_product``, float64 oracle
``inference.kf_tools.product_blocks``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from statistics import NormalDist

import numpy as np

TRANSFORM_KINDS = ("identity", "linear", "neglog")
INF = float("inf")


@dataclass(frozen=True)
class ParameterTransform:
    """``kind``: "identity" (phys = x), "linear" (phys = scale x + offset) or
    "neglog" (phys = -scale ln x, decreasing; needs 0 < lo <= hi < inf).
    ``lo`` / ``hi``: bounds in *transformed* space; every argument (the state
    and both interval ends) is clamped to them before the transform, so a
    product with finite bounds is finite by construction.  ``name``: the
    product's file / key name, ``<parameter>_phys`` when None."""
    kind: str
    scale: float = 1.0
    offset: float = 0.0
    lo: float = -INF
    hi: float = INF
    name: str | None = None
    units: str = ""

    def __post_init__(self):
        if self.kind not in TRANSFORM_KINDS:
            raise ValueError("kind must be 'identity', 'linear' or 'neglog'")
        f32 = [float(np.float32(v)) for v in (self.scale, self.offset, self.lo, self.hi)]
        if not (math.isfinite(f32[0]) and math.isfinite(f32[1])) or f32[0] == 0.0:
            raise ValueError("scale must be finite and non-zero, offset finite (in float32)")
        if not f32[2] <= f32[3]:
            raise ValueError("lo <= hi is required")
        if self.kind == "neglog" and not (f32[2] > 0.0 and math.isfinite(f32[3])):
            raise ValueError("a 'neglog' transform needs 0 < lo <= hi < inf (in float32)")

    # the float32 values the kernel and the oracle use
    def f32(self):
        """(scale, offset, lo, hi) rounded to float32, as Python floats."""
        if self.kind == "identity":
            return 1.0, 0.0, float(np.float32(self.lo)), float(np.float32(self.hi))
        off = 0.0 if self.kind == "neglog" else self.offset
        return tuple(float(np.float32(v)) for v in (self.scale, off, self.lo, self.hi))

    def apply(self, u):
        """The transform of (already clamped) ``u`` in float64."""
        u = np.asarray(u, dtype=np.float64)
        scale, offset, _, _ = self.f32()
        if self.kind == "neglog":
            with np.errstate(divide="ignore", invalid="ignore"):
                return -scale * np.log(u)
        if self.kind == "linear":
            return scale * u + offset
        return u.copy()

    def physical_range(self):
        """(min, max) of the product where ``lo`` and ``hi`` are finite (the clamp
        guarantees it), else None."""
        _, _, lo, hi = self.f32()
        if not (math.isfinite(lo) and math.isfinite(hi)):
            return None
        a, b = (float(v) for v in self.apply([lo, hi]))
        return (min(a, b) + 0.0, max(a, b) + 0.0)       # (+ 0.0: no -0.0 as a range end)

    def describe(self) -> str:
        """The ``TRANSFORM`` metadata item of a product file."""
        scale, offset, lo, hi = self.f32()
        body = {"identity": "x", "linear": f"{scale:g} * x + {offset:g}", "neglog": f"-{scale:g} * ln(x)"}[self.kind]
        return f"{body}, x clamped to [{lo:g}, {hi:g}]"


#: JRC-TIP: effective LAI from TeLAI = exp(-LAI / 2) (kf_tools.py:99-116).  hi = 1 is
#: LAI = 0 (a negative LAI has no meaning); lo = exp(-5) is LAI = 10, above any
#: effective LAI the two-stream inversion resolves (its signal saturates well below).
TIP_TRANSFORMS = {
    "TeLAI": ParameterTransform("neglog", scale=2.0, lo=math.exp(-5.0), hi=1.0, units="m2/m2"),
}

#: The SAIL state: the inverses of the prior definitions at kafka_test_S2.py:84-87
#: (exp(-cab / 100), exp(-car / 100), exp(-50 cw), exp(-100 cm), exp(-lai / 2),
#: ala / 90).  Every exponential has hi = 1 (a concentration or LAI of 0; negative
#: ones have no meaning) and lo = exp(-max / scale) with `max` the upper end of
#: the range PROSAIL is commonly run over: cab 120 ug/cm2, car 30 ug/cm2, cw
#: 0.1 cm, cm 0.05 g/cm2, lai 10 m2/m2; ala / 90 is an angle fraction in [0, 1].
#: n, cbrown, bsoil and psoil are stored untransformed and get no product.
SAIL_TRANSFORMS = {
    "cab": ParameterTransform("neglog", scale=100.0, lo=math.exp(-120.0 / 100.0), hi=1.0, units="ug/cm2"),
    "car": ParameterTransform("neglog", scale=100.0, lo=math.exp(-30.0 / 100.0), hi=1.0, units="ug/cm2"),
    "cw": ParameterTransform("neglog", scale=1.0 / 50.0, lo=math.exp(-50.0 * 0.1), hi=1.0, units="cm"),
    "cm": ParameterTransform("neglog", scale=1.0 / 100.0, lo=math.exp(-100.0 * 0.05), hi=1.0, units="g/cm2"),
    "lai": ParameterTransform("neglog", scale=2.0, lo=math.exp(-5.0), hi=1.0, units="m2/m2"),
    "ala": ParameterTransform("linear", scale=90.0, lo=0.0, hi=1.0, units="deg"),
}

TRANSFORM_TABLES = {"tip": TIP_TRANSFORMS, "sail": SAIL_TRANSFORMS}

#: QA byte of a product run (csrc/kf_core.h pixel_product); 255 outside the state mask
QA_LEGEND = (
    "bit 0: no observation assimilated in the timestep (none present, or every one rejected by the innovation gate)",
    "bit 1: the analysis fell back (not SPD, not finite or a failed operator)",
    "bit 2: an emulator input outside its training domain",
    "bit 3: an observation rejected by the innovation gate",
    "bit 4: credible interval unavailable (NaN)",
    "bit 5: state outside the transform's bounds (median clamped)",
    "bit 6: an interval end clamped to the transform's bounds",
    "bit 7: 0",
)
QA_FILL = 255


def credible_z(level) -> float:
    """z = Phi^-1((1 + level) / 2) of a central credible level in (0, 1):
    float64, rounded once to float32."""
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError("level must lie in (0, 1)")
    return float(np.float32(NormalDist().inv_cdf(0.5 * (1.0 + level))))


def product_name(parameter, transform) -> str:
    return transform.name if transform.name is not None else f"{parameter}_phys"


def resolve_products(parameter_list, physical):
    """The products of an output: [(j, name, transform)] in state order for the
    parameters of ``parameter_list`` that ``physical`` (a mapping parameter ->
    ParameterTransform, or None) has an entry for.  A product name must differ
    from every parameter name (ignoring case) and from every other product."""
    if physical is None:
        return []
    if not hasattr(physical, "items"):
        raise ValueError("physical: a mapping parameter -> ParameterTransform")
    taken = {str(p).lower() for p in parameter_list}
    out, seen = [], set()
    for j, p in enumerate(parameter_list):
        t = physical.get(p)
        if t is None:
            continue
        if not isinstance(t, ParameterTransform):
            raise ValueError(f"physical[{p!r}] is not a ParameterTransform")
        name = product_name(p, t)
        if name.lower() in taken:
            raise ValueError(f"product name {name!r} collides with a parameter of the output")
        if name.lower() in seen:
            raise ValueError(f"product name {name!r} is used twice")
        seen.add(name.lower())
        out.append((j, name, t))
    return out
