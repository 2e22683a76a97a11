"""Continuous batching through the public interfaces on the CPU: serve.py's
POST /generate_one over a ``DecodeScheduler`` worker, and sample.py with
``--slots``, over a rundir that holds a config and a char tokenizer (random
weights: the loader's no-checkpoint path)."""
import pickle
import sys
import threading

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


def _client(rundir, num_slots):
    pytest.importorskip("fastapi")
    testclient = pytest.importorskip("starlette.testclient")
    from serve import build_app
    torch.manual_seed(91)                  # the random-init weights
    return testclient.TestClient(build_app(rundir, device="cpu", num_slots=num_slots))


def test_generate_one_endpoint(rundir):
    with _client(rundir, 2) as client:
        # greedy: what /generate gives for the same prompt
        for p, n in (("hello", 5), ("a", 7), ("abcdefghijklmn", 5)):
            one = client.post("/generate_one", json={"prompt": p, "max_new_tokens": n,
                                                     "temperature": 0.0})
            assert one.status_code == 200, one.text
            ref = client.post("/generate", json={"prompt": p, "max_new_tokens": min(n, 16 - len(p) + 1),
                                                 "temperature": 0.0, "num_samples": 1})
            assert one.json() == {"sample": ref.json()["samples"][0]}
        # four requests from four threads: each returns what it returns alone
        reqs = [{"prompt": p, "max_new_tokens": n, "temperature": 1.0, "top_k": 5, "seed": 40 + i}
                for i, (p, n) in enumerate((("a", 9), ("hello", 4), ("abcdefgh", 6), ("xyz", 11)))]
        alone = [client.post("/generate_one", json=r).json()["sample"] for r in reqs]
        assert all(s.startswith(r["prompt"]) and len(s) == len(r["prompt"]) + r["max_new_tokens"]
                   for s, r in zip(alone, reqs))
        got = [None] * 4

        def post(i):
            got[i] = client.post("/generate_one", json=reqs[i]).json()["sample"]

        threads = [threading.Thread(target=post, args=(i,)) for i in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert got == alone
        # eos_id ends a request at its first such token
        eos = ALPHABET.index(alone[1][len("hello")])
        r = client.post("/generate_one", json=dict(reqs[1], eos_id=eos))
        assert r.json()["sample"] == alone[1][:len("hello") + 1]
        assert client.post("/generate_one", json={"prompt": ""}).status_code == 422
        assert client.get("/healthz").json()["status"] == "ok"


def test_generate_one_without_slots_is_503_and_the_rest_is_unchanged(rundir):
    client = _client(rundir, 0)
    assert client.post("/generate_one", json={"prompt": "a"}).status_code == 503
    # the seeded text of /generate_batch, recorded from the commit before
    # continuous batching
    r = client.post("/generate_batch", json={"prompts": ["a", "hello", "abcdefghijklmn"],
                                             "max_new_tokens": 6, "temperature": 1.0,
                                             "top_k": 5, "seed": 3})
    assert r.json() == {"samples": ["alCynJJ", "hellouJJmJJ", "abcdefghijklmnnJd"]}


def test_sample_cli_slots(rundir, tmp_path, monkeypatch, capsys):
    import sample

    def run(*extra):
        monkeypatch.setattr(sys, "argv", [
            "sample.py", f"--ckpt_dir={rundir}", "--start=a", "--start=hello", "--start=abc",
            "--max_new_tokens=4", "--temperature=0", "--seed=0", *extra])
        torch.manual_seed(91)
        sample.main()
        out = capsys.readouterr().out.split("---------------\n")
        lines = [s.rstrip("\n") for s in out[:-1]]
        lines[0] = lines[0].split("\n")[-1]    # the loader's message comes first
        return lines

    ragged = run()
    slots = run("--slots=2")
    assert len(slots) == 3 and slots == ragged
    for got, p in zip(slots, ["a", "hello", "abc"]):
        assert got.startswith(p) and len(got) == len(p) + 4, (got, p)
