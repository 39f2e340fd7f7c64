"""tools/plan_digest.py says something: equal plans give equal digests, and a flag, a shape or a wrong blob name does not go unnoticed."""
import importlib.util
import os

import pytest

from conftest import REPO

spec = importlib.util.spec_from_file_location("plan_digest", os.path.join(REPO, "tools", "plan_digest.py"))
pd = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pd)

SHAPE = (2, 45, 70)


def test_two_instances_agree():
    a, b = pd.build("RFDN", "bf16"), pd.build("RFDN", "bf16")
    assert a is not b and pd.plan_digest(a, SHAPE) == pd.plan_digest(b, SHAPE)
    assert pd.packed_digest(a) == pd.packed_digest(b)


def test_flag_and_shape_change_the_digest():
    base = pd.plan_digest(pd.build("RFDN", "bf16"), SHAPE)
    assert pd.plan_digest(pd.build("RFDN", "bf16", "fuse_esa_lowres"), SHAPE)[3] != base[3]
    assert pd.plan_digest(pd.build("RFDN", "bf16"), (2, 45, 71))[3] != base[3]


def test_missing_blob_name_raises():
    m = pd.build("RFDN", "bf16")
    names = sorted(m._packed)
    assert pd.plan_digest(m, SHAPE, names) == pd.plan_digest(m, SHAPE)
    with pytest.raises(KeyError):
        pd.plan_digest(m, SHAPE, [n for n in names if n != "B2.c5#s16"])
