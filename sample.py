"""Sampling / inference — contract parity with the reference sample.py:
``python sample.py --ckpt_dir=RUNDIR [--start=STR] [--num_samples N]
[--max_new_tokens M] [--temperature T]``

``--start`` may be given several times, or ``--start_file`` names a file with
one prompt per line: more than one prompt decodes as one ragged batch
(``generate_ragged``), one sample per prompt, ``--num_samples`` ignored; with
``--slots N`` they go through ``generate_continuous`` on N cache slots instead
(continuous batching: there may be more prompts than slots), and with
``--pages P [--page_size PS]`` on a paged cache of P pages shared by the slots.

Loads config.json + the latest checkpoint from the rundir, rebuilds the
model, and generates. Improvement over the reference (which re-runs a full
forward per new token, sample.py:68-95): an incremental KV cache decode.
"""
from __future__ import annotations

import argparse
import os
import pickle

import torch

from midgpt_amd import ops
from midgpt_amd.config import ExperimentConfig
from midgpt_amd.generate import generate, generate_continuous, generate_ragged
from midgpt_amd.models.gpt import GPT
from midgpt_amd.utils import checkpoint as ckpt


def load_model(ckpt_dir: str, device: torch.device) -> tuple[GPT, ExperimentConfig]:
    with open(os.path.join(ckpt_dir, "config.json")) as f:
        config = ExperimentConfig.from_json(f.read())
    model = GPT(config.model_config)
    state = ckpt.load_full_state(ckpt_dir)
    if state is not None:
        master = state["master"]
        sd = {}
        for pm in state["manifest"]["params"]:
            n, shape = pm["numel"], pm["shape"]
            sd[pm["name"]] = master[pm["offset"]:pm["offset"] + n].view(shape)
        # strict=False only because rope sin/cos buffers are non-persistent
        missing, unexpected = model.load_state_dict(sd, strict=False)
        assert not unexpected, f"unexpected checkpoint params: {unexpected}"
        print(f"loaded checkpoint step {state['step']}")
    else:
        print("no checkpoint found; using random init")
    model = model.to(device)
    if device.type == "cuda":
        model = model.to(torch.bfloat16)
        # rope tables stay fp32
        model.rope_sin = model.rope_sin.float()
        model.rope_cos = model.rope_cos.float()
    model.eval()
    return model, config


def load_model_and_tokenizer(ckpt_dir: str, device):
    """Model + encode/decode fns for a rundir (tokenizer: char meta.pkl
    if the config's data_dir has one, else tiktoken GPT-2 — reference
    sample.py:143-159)."""
    device = torch.device(device) if not isinstance(device, torch.device) \
        else device
    model, config = load_model(ckpt_dir, device)
    meta_path = os.path.join(config.data_dir, "meta.pkl")
    if os.path.exists(meta_path):
        with open(meta_path, "rb") as f:
            meta = pickle.load(f)
        encode = lambda s: [meta["stoi"][c] for c in s]  # noqa: E731
        decode = lambda t: "".join(meta["itos"][i] for i in t)  # noqa: E731
    else:
        try:
            import tiktoken
        except ImportError as e:
            raise SystemExit(
                "no meta.pkl in the config's data_dir and tiktoken is not "
                "installed (offline image): token-id I/O only — rerun with "
                "a char-level dataset or install tiktoken") from e
        enc = tiktoken.get_encoding("gpt2")
        encode = lambda s: enc.encode(s, allowed_special={"<|endoftext|>"})  # noqa: E731
        decode = enc.decode
    return model, encode, decode, config


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ckpt_dir", required=True)
    p.add_argument("--start", action="append", default=None,
                   help="prompt; repeat for a batch of different prompts")
    p.add_argument("--start_file", default=None,
                   help="file with one prompt per line")
    p.add_argument("--top_k", type=int, default=None)
    p.add_argument("--eos_id", type=int, default=None,
                   help="ragged batch only: end a sample at this token id")
    p.add_argument("--num_samples", type=int, default=3)
    p.add_argument("--max_new_tokens", type=int, default=200)
    p.add_argument("--temperature", type=float, default=0.8)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--slots", type=int, default=0,
                   help="several prompts: decode them by continuous batching on "
                        "this many cache slots (0: one ragged batch)")
    p.add_argument("--pages", type=int, default=None,
                   help="with --slots: a paged cache of this many pages shared by "
                        "the slots (default: one whole cache per slot)")
    p.add_argument("--page_size", type=int, default=16,
                   help="with --pages: positions per page, a power of two in [16, 128]")
    args = p.parse_args()
    if args.pages is not None and args.slots <= 0:
        p.error("--pages needs --slots N")

    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model, encode, decode, config = load_model_and_tokenizer(args.ckpt_dir,
                                                             device)

    # seeded sampling (ops.sample_tokens): one --seed, one text, on the CPU
    # and on the GPU alike; without one a seed is drawn
    seed = ops.draw_sample_seed() if args.seed is None else args.seed
    starts = list(args.start or [])
    if args.start_file is not None:
        with open(args.start_file) as f:
            starts += [line.rstrip("\n") for line in f if line.strip()]
    if len(starts) > 1:
        prompts = [torch.tensor(encode(s), dtype=torch.int64, device=device)
                   for s in starts]
        if args.slots > 0:
            outs = generate_continuous(model, prompts, args.max_new_tokens,
                                       temperature=args.temperature, top_k=args.top_k,
                                       eos_id=args.eos_id, num_slots=args.slots, seed=seed,
                                       num_pages=args.pages, page_size=args.page_size)
        else:
            outs = generate_ragged(model, prompts, args.max_new_tokens,
                                   temperature=args.temperature, top_k=args.top_k,
                                   eos_id=args.eos_id, seed=seed)
        for o in outs:
            print(decode(o.tolist()))
            print("---------------")
        return
    start = starts[0] if starts else "\n"
    prompt = torch.tensor(encode(start), dtype=torch.int64, device=device)
    prompt = prompt.unsqueeze(0).expand(args.num_samples, -1)
    out = generate(model, prompt, args.max_new_tokens,
                   temperature=args.temperature, seed=seed)
    for i in range(args.num_samples):
        print(decode(out[i].tolist()))
        print("---------------")


if __name__ == "__main__":
    main()
