"""Minimal text-generation serving endpoint over a trained checkpoint.

Beyond the reference's scope (midGPT has only offline sample.py —
reference sample.py:29-37); included because this framework targets
production serving as well as pretraining. Loads a rundir checkpoint the
same way sample.py does, then serves batched KV-cache generation
(midgpt_amd/generate.py) over HTTP.

    python serve.py --ckpt_dir runs/xl [--host 127.0.0.1 --port 8000] [--slots N]
                    [--pages P [--page_size PS]]

    POST /generate {"prompt": "...", "max_new_tokens": 200,
                    "temperature": 0.8, "top_k": null, "num_samples": 1,
                    "seed": null}
    POST /generate_batch {"prompts": ["...", "..."], "max_new_tokens": 200,
                          "temperature": 0.8, "top_k": null, "seed": null,
                          "eos_id": null}
         different prompts decoded together (generate_ragged): one sample per
         prompt, each at most block_size tokens long with its prompt (no
         sliding window), cut after its first eos_id if that is given
    POST /generate_one {"prompt": "...", "max_new_tokens": 200,
                        "temperature": 0.8, "top_k": null, "seed": null,
                        "eos_id": null}
         with --slots N > 0: the request joins the running batch of a
         DecodeScheduler with N cache slots (continuous batching), so
         concurrent requests share decode steps; returns {"sample": "..."}.
         Limits as for /generate_batch. With --slots 0 (the default): 503.
         With --pages P the scheduler's cache is paged: N seats share P pages
         of --page_size positions (default 16) and a request holds only the
         pages it can write; one that needs more than P pages is refused
    GET  /healthz

Sampling is seeded (``ops.sample_tokens``): "seed" fixes the text of a
request, on the CPU and on the GPU alike; without one a seed is drawn from
torch's CPU generator.
"""
import argparse
import collections
import contextlib
import threading

import torch

from sample import load_model_and_tokenizer


def _seed_of(seed):
    """The request's seed, or a fresh one: sampling stays on the device."""
    from midgpt_amd import ops
    return ops.draw_sample_seed() if seed is None else seed


class _Job:
    """One /generate_one request on its way through the worker."""

    def __init__(self, prompt, kw):
        self.prompt, self.kw = prompt, kw
        self.finished = threading.Event()
        self.handle = None
        self.error = None


class SchedulerWorker:
    """One thread that owns a ``DecodeScheduler`` and is the only one to touch
    it: it takes new requests from an inbox between two steps, steps while
    there is work and sleeps on a condition otherwise. ``generate`` may be
    called from any number of threads and blocks until its request is done."""

    def __init__(self, model, num_slots: int, num_pages: int | None = None,
                 page_size: int = 16):
        from midgpt_amd.generate import DecodeScheduler
        self.sched = DecodeScheduler(model, num_slots, num_pages=num_pages,
                                     page_size=page_size)
        self.inbox = collections.deque()
        self.wake = threading.Condition()
        self.closed = None        # the reason, once the thread is to end
        self.thread = threading.Thread(target=self._loop, daemon=True,
                                       name="decode-scheduler")
        self.thread.start()

    def _loop(self):
        running = {}              # id(handle) -> job
        while True:
            with self.wake:
                while not self.inbox and not running and self.closed is None:
                    self.wake.wait()
                if self.closed is not None:
                    break
                jobs = list(self.inbox)
                self.inbox.clear()
            try:
                for job in jobs:
                    try:
                        job.handle = self.sched.submit(job.prompt, **job.kw)
                        running[id(job.handle)] = job
                    except (RuntimeError, ValueError) as e:   # a bad request
                        job.error = e
                        job.finished.set()
                for handle in self.sched.step():
                    running.pop(id(handle)).finished.set()
            except Exception as e:         # the scheduler itself: fail every waiter
                with self.wake:
                    self.closed = e
                break
        with self.wake:
            stranded = list(running.values()) + list(self.inbox)
            self.inbox.clear()
        for job in stranded:
            job.error = RuntimeError(f"decode scheduler stopped: {self.closed!r}")
            job.finished.set()

    def close(self):
        """End the thread after the step it is in; waiting requests fail."""
        with self.wake:
            if self.closed is None:
                self.closed = "closed"
            self.wake.notify()
        self.thread.join()

    def generate(self, prompt, **kw):
        job = _Job(prompt, kw)
        with self.wake:
            if self.closed is not None:
                raise RuntimeError(f"decode scheduler stopped: {self.closed!r}")
            self.inbox.append(job)
            self.wake.notify()
        job.finished.wait()
        if job.error is not None:
            raise job.error
        return job.handle.tokens


def build_app(ckpt_dir: str, device: str | None = None, num_slots: int = 0,
              num_pages: int | None = None, page_size: int = 16):
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

    class OneRequest(BaseModel):
        prompt: str = "\n"
        max_new_tokens: int = 200
        temperature: float = 0.8
        top_k: int | None = None
        seed: int | None = None
        eos_id: int | None = None

    worker = SchedulerWorker(model, num_slots, num_pages, page_size) \
        if num_slots > 0 else None

    @contextlib.asynccontextmanager
    async def lifespan(app):
        yield
        if worker is not None:
            worker.close()

    app = FastAPI(title="midgpt_amd", lifespan=lifespan)

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

    @app.post("/generate_one")
    def generate_one_ep(req: OneRequest):
        from fastapi import HTTPException
        if worker is None:
            raise HTTPException(status_code=503,
                                detail="continuous batching is off: start with --slots N")
        prompt = torch.tensor(encode(req.prompt), dtype=torch.long, device=device)
        if prompt.numel() == 0:
            raise HTTPException(status_code=422, detail="empty prompt")
        out = worker.generate(prompt, max_new_tokens=req.max_new_tokens,
                              temperature=req.temperature, top_k=req.top_k,
                              seed=_seed_of(req.seed), eos_id=req.eos_id)
        return {"sample": decode(out.tolist())}

    return app


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt_dir", required=True)
    p.add_argument("--host", default="127.0.0.1")
    p.add_argument("--port", type=int, default=8000)
    p.add_argument("--slots", type=int, default=0,
                   help="cache slots of the continuous-batching scheduler behind "
                        "/generate_one (0: off)")
    p.add_argument("--pages", type=int, default=None,
                   help="with --slots: page the scheduler's cache, this many pages "
                        "shared by the slots (default: one whole cache per slot)")
    p.add_argument("--page_size", type=int, default=16,
                   help="with --pages: positions per page, a power of two in [16, 128]")
    args = p.parse_args()
    if args.pages is not None and args.slots <= 0:
        p.error("--pages needs --slots N")
    import uvicorn
    uvicorn.run(build_app(args.ckpt_dir, num_slots=args.slots, num_pages=args.pages,
                          page_size=args.page_size), host=args.host, port=args.port)


if __name__ == "__main__":
    main()
