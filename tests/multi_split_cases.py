"""The fixtures and the launch forcing shared by the packed split kernel's GPU
tests (tests/test_multi_split_*_gpu.py): every case runs
k_step_split_multi<pol, block, false, 0, true, fast> (csrc/sk_multi.hpp), on
64- and 512-lane workgroups, through the plain and the write-through port, on
the fp64 carry and the fp32-trig tick.  tests/test_multi_plan_cpu.py pins that
this forcing reaches exactly that instantiation.
"""
import pytest


@pytest.fixture(params=["64", "512"], ids=["block64", "block512"])
def block(request):
    return request.param


@pytest.fixture(params=[0, 1], ids=["plain", "write_through"])
def pol(request):
    return request.param


@pytest.fixture(params=["0", "1"], ids=["fp64carry", "fast"])
def fast(request):
    return request.param


def _env(monkeypatch, pol, block, fast):
    monkeypatch.setenv("SK_MULTI_SPLIT", "1")
    monkeypatch.setenv("SK_MULTI_PACK", "1")
    monkeypatch.setenv("SK_MULTI_FAST", fast)
    monkeypatch.setenv("SK_MULTI_POLICY", str(pol))
    monkeypatch.setenv("SK_MULTI_BLOCK", block)
