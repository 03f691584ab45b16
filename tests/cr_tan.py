"""Correctly rounded fp64 tan, sin and cos by 70-digit Decimal arithmetic (test infrastructure).

float(Decimal) rounds correctly, so cr_tan(x) is the fp64 value nearest the
exact tan of the double x (cr_sin, cr_cos alike).  Used to pin csrc/sk_tan_cr.hpp,
to classify the probe boards where glibc's math.tan (the reference's) is not
correctly rounded, and as the independent reference of the device numerics
tests (tests/test_device_numerics_gpu.py).
"""
from decimal import Decimal, localcontext

_PI = Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899862803482534211706798")
_EPS = Decimal(10) ** -72


def _reduced_sin_cos(x):
    """(k, sin r, cos r) as Decimals with x = k * pi/2 + r, |r| <= pi/4; call under a prec-80 context"""
    d = Decimal(float(x))
    k = (d / (_PI / 2)).to_integral_value()
    r = d - k * (_PI / 2)
    r2 = r * r
    s, term, i = Decimal(0), r, 1
    while abs(term) > _EPS * abs(r):  # relative to r: a subnormal x keeps its sine
        s += term
        term = -term * r2 / ((2 * i) * (2 * i + 1))
        i += 1
    c, term, i = Decimal(0), Decimal(1), 1
    while abs(term) > _EPS:
        c += term
        term = -term * r2 / ((2 * i - 1) * (2 * i))
        i += 1
    return int(k), s, c


def cr_tan(x):
    with localcontext() as ctx:
        ctx.prec = 80
        k, s, c = _reduced_sin_cos(x)
        t = -c / s if k % 2 else s / c
        return float(t)


def cr_sincos(x):
    """(sin x, cos x), each correctly rounded to fp64; sin(+-0) = +-0"""
    if x == 0:
        return float(x), 1.0
    with localcontext() as ctx:
        ctx.prec = 80
        k, s, c = _reduced_sin_cos(x)
        q = k % 4
        return float((s, c, -s, -c)[q]), float((c, -s, -c, s)[q])


def cr_sin(x):
    return cr_sincos(x)[0]


def cr_cos(x):
    return cr_sincos(x)[1]
