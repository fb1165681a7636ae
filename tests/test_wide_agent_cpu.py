"""CPU self-check of the wide-encoder agent test (tests/wide_agent_models.py; tests/test_gpu_wide_agent.py runs the
product against the same oracle runs): the seed is the first whose smallest top-two perturbed-logit margin under the
float32 oracle is >= 1e-4 and whose float32 and float64 oracles draw the same posterior and imagined indices, so the
GPU test can demand exact index equality; and the float32 oracle sits inside the GPU test's loss bound."""
import numpy as np
import torch

import wide_agent_models as wa


def test_the_case_crosses_128_channels_in_two_stages():
    spec, params = wa.spec_params(wa.SEED)
    widths = [params[f"encoder.encoders.0.layers.{4 * i}.weight"].shape[:2] for i in range(4)]
    assert [tuple(w) for w in widths] == [(66, 3), (99, 66), (132, 99), (132, 132)]
    assert spec.E == 132 * 16
    d, init = wa.inputs(wa.SEED, 0)
    assert d["image"].shape == (wa.B, wa.T, 64, 64, 3) and d["is_first"][:, 0].all() and d["is_first"][1, 2]
    assert not np.array_equal(wa.inputs(wa.SEED, 0)[0]["image"], wa.inputs(wa.SEED, 1)[0]["image"])


def test_the_seed_is_the_first_that_meets_the_input_condition():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    assert wa.SEED < wa.MAX_SEEDS and wa.meets_condition(wa.SEED)
    for s in range(wa.SEED):
        assert not wa.meets_condition(s), f"seed {s} meets the condition too"
    r32, r64 = wa.run_oracle(wa.SEED, torch.float32), wa.run_oracle(wa.SEED, torch.float64)
    print("margins", [r["margin"] for r in r32])
    for a, b in zip(r32, r64):  # the float32 oracle against float64 on the GPU test's world-model loss bound
        for k in wa.WM_KEYS:
            assert abs(a["losses"][k] - b["losses"][k]) <= 1e-4 * max(abs(b["losses"][k]), 1e-6) + 1e-6, k
