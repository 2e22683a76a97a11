"""Minimal text-generation serving endpoint over a trained checkpoint.

Beyond the reference's scope (midGPT has only offline sample.py —
reference sample.py:29-37); included because this framework targets
production serving as well as pretraining. Loads a rundir checkpoint the
same way sample.py does, then serves batched KV-cache generation
(midgpt_amd/generate.py) over HTTP.

    python serve.py --ckpt_dir runs/xl [--host 127.0.0.1 --port 8000]

    POST /generate {"prompt": "...", "max_new_tokens": 200,
                    "temperature": 0.8, "top_k": null, "num_samples": 1,
                    "seed": null}
    POST /generate_batch {"prompts": ["...", "..."], "max_new_tokens": 200,
                          "temperature": 0.8, "top_k": null, "seed": null,
                          "eos_id": null}
         different prompts decoded together (generate_ragged): one sample per
         prompt, each at most block_size tokens long with its prompt (no
         sliding window), cut after its first eos_id if that is given
    GET  /healthz

Sampling is seeded (``ops.sample_tokens``): "seed" fixes the text of a
request, on the CPU and on the GPU alike; without one a seed is drawn from
torch's CPU generator.
"""
import argparse

import torch

from sample import load_model_and_tokenizer


def _seed_of(seed):
    """The request's seed, or a fresh one: sampling stays on the device."""
    from midgpt_amd import ops
    return ops.draw_sample_seed() if seed is None else seed


def build_app(ckpt_dir: str, device: str | None = None):
    from fastapi import FastAPI
    from pydantic import BaseModel

    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    model, encode, decode, config = load_model_and_tokenizer(ckpt_dir, device)

    class GenRequest(BaseModel):
        prompt: str = "\n"
        max_new_tokens: int = 200
        temperature: float = 0.8
        top_k: int | None = None
        num_samples: int = 1
        seed: int | None = None

    class BatchRequest(BaseModel):
        prompts: list[str]
        max_new_tokens: int = 200
        temperature: float = 0.8
        top_k: int | None = None
        seed: int | None = None
        eos_id: int | None = None

    app = FastAPI(title="midgpt_amd")

    @app.get("/healthz")
    def healthz():
        return {"status": "ok", "device": device,
                "block_size": config.model_config.block_size}

    @app.post("/generate")
    def generate_ep(req: GenRequest):
        from midgpt_amd.generate import generate
        ids = encode(req.prompt)
        idx = torch.tensor([ids] * req.num_samples, dtype=torch.long,
                           device=device)
        out = generate(model, idx, req.max_new_tokens,
                       temperature=req.temperature, top_k=req.top_k,
                       seed=_seed_of(req.seed))
        return {"samples": [decode(out[i].tolist())
                            for i in range(req.num_samples)]}

    @app.post("/generate_batch")
    def generate_batch_ep(req: BatchRequest):
        from fastapi import HTTPException
        from midgpt_amd.generate import generate_ragged
        prompts = [torch.tensor(encode(p), dtype=torch.long, device=device)
                   for p in req.prompts]
        if any(p.numel() == 0 for p in prompts):
            raise HTTPException(status_code=422, detail="empty prompt")
        outs = generate_ragged(model, prompts, req.max_new_tokens,
                               temperature=req.temperature, top_k=req.top_k,
                               eos_id=req.eos_id, seed=_seed_of(req.seed))
        return {"samples": [decode(o.tolist()) for o in outs]}

    return app


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt_dir", required=True)
    p.add_argument("--host", default="127.0.0.1")
    p.add_argument("--port", type=int, default=8000)
    args = p.parse_args()
    import uvicorn
    uvicorn.run(build_app(args.ckpt_dir), host=args.host, port=args.port)


if __name__ == "__main__":
    main()
