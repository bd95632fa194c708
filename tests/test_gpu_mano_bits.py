"""The MANO kernels (csrc/mano_lbs.hip) against the recorded bits of the kernels as they were while each entry-point pair
had its own template instantiations: tests/golden/mano_bits.json holds, per case, a SHA-256 of the raw bytes of every input
and of every output -- verts, joints, grad pose, grad betas, grad trans -- computed on an MI355X through
``SynthManoLayer.forward`` / ``forward_full``.

tests/test_gpu_mano_grads.py compares the kernels with an fp64 oracle under a yardstick and the two entry points with each
other; a change that moves both entry points' bits together passes there and fails here.  The cases are those of
tests/geom_grad_cases.py (every variant x run x weight pattern) and the three epilogue cases of test_gpu_mano_full.py
(tests/golden/make_golden_mano_bits.py lists them).  The file is never regenerated from later code: a differing output
digest is a changed result, to be found by reading which expression, order or launch changed."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_golden_mano_bits", os.path.join(GOLDEN, "make_golden_mano_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "mano_bits.json")) as _fh:
    RECORD = json.load(_fh)


def test_record_covers_every_case():
    """No GPU: the record has exactly the generator's cases -- every variant x run x weight pattern of geom_grad_cases and
    the three epilogue cases --, every digest is one, and the record names the library it was taken from"""
    from tests import geom_grad_cases as C

    assert len(gen.GRAD_CASES) == len(C.MANO_VARIANTS) * len(C.MANO_RUNS) * len(C.MANO_WEIGHTS)
    assert len(set(gen.CASES)) == len(gen.CASES) == len(gen.GRAD_CASES) + 3
    assert set(RECORD["cases"]) == set(gen.CASES)
    assert len(RECORD["source_hash"]) == 64
    hexdigits = set("0123456789abcdef")
    for name, rec in RECORD["cases"].items():
        assert {"pose", "betas"} <= set(rec["inputs"]) and {"verts", "joints"} <= set(rec["outputs"]), name
        if not name.startswith("epilogue-"):
            want = {"grad pose", "grad betas"} | ({"grad trans"} if "trans" in rec["inputs"] else set())
            assert want <= set(rec["outputs"]), name
        assert all(len(v) == 64 and set(v) <= hexdigits for part in rec.values() for v in part.values()), name


@pytest.mark.gpu
@pytest.mark.parametrize("case", gen.CASES)
def test_bits_equal_the_record(cuda, case):
    rec = RECORD["cases"][case]
    ins, outs = gen.digests(case, cuda)
    assert ins == rec["inputs"], (f"{case}: the case changed, not the kernel -- inputs "
                                  f"{sorted(k for k in set(ins) | set(rec['inputs']) if ins.get(k) != rec['inputs'].get(k))} differ from the record")
    differ = sorted(k for k in set(outs) | set(rec["outputs"]) if outs.get(k) != rec["outputs"].get(k))
    assert not differ, f"{case}: {differ} differ from the recorded bits"
