"""Multi-GPU (RCCL): under ZeRO every transposed weight image equals
``weight.t()`` on every rank after a step's all-gather. Skipped unless >=2
GPUs are visible, as tests/test_multigpu.py; the 1-GPU twin over gloo is
test_gpu_dgrad_wt.py::test_zero_two_ranks_one_gpu_images."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.gpu8]

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not torch.cuda.is_available() or
                    torch.cuda.device_count() < 2,
                    reason="needs >=2 GPUs")
def test_multigpu_zero_images_equal_transpose():
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.pop("MIDGPT_DGRAD_WT", None)
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node=2", "--master-addr=127.0.0.1",
         "--master-port=29774",
         os.path.join(REPO, "tests", "_mgpu_dgrad_wt_worker.py")],
        env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    assert (r.stdout + r.stderr).count("DGRAD-WT-ZERO-OK") == 2
