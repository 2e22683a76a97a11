"""Exact checks of the training engine on the CPU (synchronous path): the
scripted-gradient toy of engine_util through ShardedAdamW, world 1 and two
gloo ranks. The accumulated gradient has one right value per element, so
g32 is compared bit for bit; the update is held to the per-element fp64
bound of kernel_edge_util.adamw_figures; flat_w must be the bf16 image of
the assembled master. test_gpu_engine_exact.py runs the same harness
through the overlap pipeline on the GPU.
"""
import pytest

import engine_util as E
from midgpt_amd.parallel.engine import ShardedAdamW


@pytest.mark.parametrize("presence,K", [("all", 1), ("all", 3), ("missing", 3)])
@pytest.mark.parametrize("clip", [1.0, 1e30])
@pytest.mark.parametrize("n_buckets", [1, 7])
def test_world1_exact(n_buckets, clip, presence, K):
    toy = E.Toy()
    engine = ShardedAdamW(toy, compute_dtype=E.BF, zero=True,
                          grad_clip=clip, n_buckets=n_buckets)
    assert not engine.zero and engine.n_buckets == n_buckets
    assert engine.buckets == E.bucket_layout(E.TOTAL, 1, False, n_buckets)[1]
    script = E.Script(K, 1, presence, "forward")
    out = E.run_steps(engine, toy, script, range(3),
                      tag=f"cpu w1 nb{n_buckets} K{K} clip{clip:g} {presence}")
    assert len(out) == 3 and engine.step_count == 3


# ---------------------------------------------------------------------------
# two ranks over gloo
# ---------------------------------------------------------------------------
# (zero, n_buckets, clip). With clip 1.0 these gradients are clipped hard and
# grad_scale cancels out of the update; only 1e30 shows a wrong scale.
SCENARIOS_W2 = [(True, 1, 1.0), (True, 7, 1e30), (False, 1, 1e30), (False, 7, 1.0)]


def test_world2_gloo_exact(tmp_path):
    stuck, codes = E.run_pair(tmp_path, SCENARIOS_W2, "cpu", record=False)
    assert not stuck, "a worker was still running at the timeout"
    assert codes == [0, 0], codes
    E.check_pair(tmp_path, SCENARIOS_W2)
