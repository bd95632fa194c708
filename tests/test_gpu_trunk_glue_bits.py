"""The trunk's glue kernels (csrc/frozen_bn.hip, csrc/stem_pool.hip on csrc/bn_device.hpp) against the recorded bits of
the kernels as they were before they shared a device layer: tests/golden/trunk_glue_bits.json holds, per case, a SHA-256
of the raw bytes of every input and every output -- y, the stem's codes / records, grad_x, grad_residual, grad_xd,
grad_weight, grad_bias and the downsample pair -- computed on an MI355X through the raw entry points.

The data are random normal values (tests/golden/make_golden_trunk_glue.py says how they are drawn and which kernel
instantiation and reduction stage each case reaches), so products and sums round and a changed expression shape,
summation order, grid size or slot count changes a digest; the exact tests next to this one cannot see those.  The file
is never regenerated from later code: a differing output digest is a changed result, to be found by reading which
helper changed an expression or an order."""
import importlib.util
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_golden_trunk_glue", os.path.join(GOLDEN, "make_golden_trunk_glue.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "trunk_glue_bits.json")) as _fh:
    RECORD = json.load(_fh)


def test_record_covers_every_case():
    """No GPU: the record has exactly the generator's cases, each in fp32 and bf16, and names the library it was taken from"""
    want = {f"{c.name}-{tag}" for c in gen.CASES for tag in gen.DTYPES}
    assert set(RECORD["cases"]) == want
    assert len(RECORD["source_hash"]) == 64
    for name, rec in RECORD["cases"].items():
        assert rec["inputs"] and rec["outputs"], name
        assert all(len(v) == 64 for part in rec.values() for v in part.values()), name


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(gen.DTYPES))
@pytest.mark.parametrize("case", gen.CASES, ids=lambda c: c.name)
def test_bits_equal_the_record(cuda, case, tag):
    rec = RECORD["cases"][f"{case.name}-{tag}"]
    ins, outs = gen.digests(case, gen.DTYPES[tag], cuda)
    assert ins == rec["inputs"], (f"{case.name} {tag}: the generator changed, not the kernel -- inputs "
                                  f"{sorted(k for k in set(ins) | set(rec['inputs']) if ins.get(k) != rec['inputs'].get(k))} differ from the record")
    differ = sorted(k for k in set(outs) | set(rec["outputs"]) if outs.get(k) != rec["outputs"].get(k))
    assert not differ, f"{case.name} {tag}: {differ} differ from the recorded bits"
