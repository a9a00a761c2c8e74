"""CPU: the cases of tests/test_gpu_decoder_family.py (tests/decoder_family.py) are not empty -- with the bias-shift construction
every shape's oracle iteration has a render term of at least 100 rows over at least 1000 valid samples, in float64 and in float32
alike -- and the float64 evaluation of the oracle is the float32 one to float32 rounding."""
import numpy as np

from oracle import sdf_oracle as so
from tests import decoder_family as fam
from tests.test_oracle_sdf import relerr


def test_every_family_case_has_a_render_term():
    assert len(fam.SHAPES) >= 10
    for name in fam.SHAPES:
        case = fam.build_case(name)
        it, it32 = case["it"], fam.oracle_iteration(case, f64=False)
        assert it["fail"] is None and it["K"] >= 100 and it["n_valid"] >= 1000, (name, it["fail"], it.get("K"), it.get("n_valid"))
        assert it["H"].dtype == np.float64 and it32["H"].dtype == np.float32
        assert it32["fail"] is None and it32["K"] == it["K"] and it32["n_valid"] == it["n_valid"], name
        assert it["H"].shape == (7 + case["L"],) * 2 and it["code_new"].shape == (case["L"],)
        # (measured: 6e-7 / 5e-6 at most; the bar of the GPU tests is 1e-4)
        assert relerr(it32["H"], it["H"]) < 1e-5 and relerr(it32["b"], it["b"]) < 1e-5, name
        r_margin, s_margin = fam.decision_margins(case)
        assert r_margin > 2e-5 and s_margin > 2e-5, (name, r_margin, s_margin)
    assert so.F32 is np.float32                     # the float64 evaluation put the oracle's working precision back
    for group in (fam.MIXED, fam.POSE_ONLY, [n for n, _ in fam.ROWS]):
        assert all(n in fam.SHAPES for n in group)
    assert len({fam.SHAPES[n][0] for n in fam.MIXED}) == 1 and all(fam.SHAPES[n][3] for n in fam.MIXED)


def test_working_precision_is_restored_after_an_exception():
    try:
        with so.working_precision(np.float64):
            assert so.F32 is np.float64
            raise KeyError("inside")
    except KeyError:
        pass
    assert so.F32 is np.float32
