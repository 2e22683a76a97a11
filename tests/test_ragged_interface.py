"""The ragged batch through the public interfaces on the CPU: serve.py's
POST /generate_batch and sample.py with several prompts, over a rundir that
holds a config and a char tokenizer (random weights: the loader's
no-checkpoint path)."""
import pickle
import sys

import pytest
import torch

from midgpt_amd.config import ExperimentConfig, GPTConfig

BLOCK = 16
ALPHABET = [chr(97 + i) for i in range(26)] + list("ABCDEFGHIJK")     # 37 chars


@pytest.fixture()
def rundir(tmp_path, monkeypatch):
    # fp32 CPU-tier model: the loaders must pick the CPU even beside a GPU
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    data_dir = tmp_path / "data"
    data_dir.mkdir()
    with open(data_dir / "meta.pkl", "wb") as f:
        pickle.dump({"vocab_size": 37,
                     "stoi": {c: i for i, c in enumerate(ALPHABET)},
                     "itos": {i: c for i, c in enumerate(ALPHABET)}}, f)
    cfg = ExperimentConfig(
        rundir=str(tmp_path / "run"), data_dir=str(data_dir), learning_rate=1e-3,
        batch_size=4, warmup_steps=2, min_lr=1e-4, lr_decay_steps=50, max_steps=2,
        beta2=0.95, weight_decay=1e-4, eval_interval=10, param_dtype="float32",
        compute_dtype="float32", g_accum_iters=1, shard_model=False,
        synthetic_data=True, seed=7,
        model_config=GPTConfig(block_size=BLOCK, vocab_size=37, n_layer=2, n_head=2,
                               n_embd=32, dropout=0.0))
    (tmp_path / "run").mkdir()
    with open(tmp_path / "run" / "config.json", "w") as f:
        f.write(cfg.to_json())
    return str(tmp_path / "run")


def test_generate_batch_endpoint(rundir):
    pytest.importorskip("fastapi")
    testclient = pytest.importorskip("starlette.testclient")
    from serve import build_app
    torch.manual_seed(81)                  # the random-init weights
    client = testclient.TestClient(build_app(rundir, device="cpu"))
    prompts = ["a", "hello", "abcdefghijklmn"]            # 1, 5, 14 of 16
    r = client.post("/generate_batch", json={"prompts": prompts, "max_new_tokens": 5,
                                             "temperature": 0.0})
    assert r.status_code == 200, r.text
    samples = r.json()["samples"]
    assert len(samples) == 3
    assert all(s.startswith(p) for s, p in zip(samples, prompts))
    # 14 + 5 > block_size 16: that sequence stops at 16 - 14 + 1 = 3 tokens
    assert [len(s) - len(p) for s, p in zip(samples, prompts)] == [5, 5, 3]
    # greedy: each sample is what /generate gives for that prompt alone
    for p, s in zip(prompts[:2], samples[:2]):
        one = client.post("/generate", json={"prompt": p, "max_new_tokens": 5,
                                             "temperature": 0.0, "num_samples": 1})
        assert one.json()["samples"] == [s]
    # eos_id: the first token the second prompt emits ends it at once
    eos = ALPHABET.index(samples[1][len(prompts[1])])
    r = client.post("/generate_batch", json={"prompts": prompts, "max_new_tokens": 5,
                                             "temperature": 0.0, "eos_id": eos})
    assert r.json()["samples"][1] == samples[1][:len(prompts[1]) + 1]
    # sampling with a seed is reproducible
    req = {"prompts": prompts, "max_new_tokens": 4, "temperature": 1.0, "top_k": 5,
           "seed": 3}
    a = client.post("/generate_batch", json=req).json()["samples"]
    assert a == client.post("/generate_batch", json=req).json()["samples"]
    assert client.post("/generate_batch", json={"prompts": ["ab", ""]}).status_code == 422
    assert client.post("/generate_batch", json={"prompts": []}).json() == {"samples": []}


def test_sample_cli_several_prompts(rundir, tmp_path, monkeypatch, capsys):
    import sample
    with open(tmp_path / "prompts.txt", "w") as f:
        f.write("hello\n\nabc\n")
    monkeypatch.setattr(sys, "argv", [
        "sample.py", f"--ckpt_dir={rundir}", "--start=a",
        f"--start_file={tmp_path / 'prompts.txt'}", "--max_new_tokens=4",
        "--temperature=0", "--seed=0"])
    torch.manual_seed(81)
    sample.main()
    out = capsys.readouterr().out.split("---------------\n")
    lines = [s.rstrip("\n") for s in out[:-1]]
    lines[0] = lines[0].split("\n")[-1]    # the loader's message comes first
    assert len(lines) == 3
    for got, p in zip(lines, ["a", "hello", "abc"]):
        assert got.startswith(p) and len(got) == len(p) + 4, (got, p)
