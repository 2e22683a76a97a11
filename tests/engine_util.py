"""Scripted-gradient harness for the training engine (test_engine_exact.py,
test_gpu_engine_exact.py). Plain torch; runs on whatever device the toy
lives on.

The engine's data path -- flat grad buffers, bucket launches, deferred fp32
accumulation, the ZeRO piece map, the weight all-gather -- moves numbers
around and adds them. With gradients that are multiples of 1/8 and sums
below 8, every one of those additions is exact in bf16 and in fp32, in any
order, so the accumulated gradient has ONE right value per element and a
dropped, doubled or misplaced piece shows as a bit difference. Only the
AdamW update itself rounds; it is held to the per-element fp64 bound of
kernel_edge_util.adamw_figures, with the exact expected gradient as input.

- ``Toy``: a ParameterList of odd shapes whose flat layout puts a parameter
  across three buckets, a bucket boundary inside a parameter, several small
  parameters inside one bucket and 1-element parameters at both ends.
- ``Script``: for (step, microstep, rank, parameter) either "absent" or a
  bf16 tensor c of multiples of 1/8 in [-1, 1]; the microbatch loss is
  sum((p * c).sum()), so the gradient of p is exactly c.
- ``check_step``: everything one optimizer step must leave behind.
- ``Recorder``: which bucket launched when, and the order the hooks fired.
- ``run_steps``: the training loop all scenarios share.
- ``run_pair`` / ``check_pair``: two spawned gloo ranks and the parent's
  view of what they left.
"""
from __future__ import annotations

import datetime
import functools
import os
import traceback

import numpy as np
import torch
import torch.nn as nn

import kernel_edge_util as U
from midgpt_amd.parallel.engine import ShardedAdamW

BF = torch.bfloat16
LR = 1e-3

# Flat offsets (total 7341733, odd; one ddp bucket of 7 is 1048819 long):
#   0        p0 (1,)           first 1-element parameter
#   1        p1 (1023, 1025)   fills bucket 0 almost to its end
#   1048576  p2 (3, 5, 7)      small, wholly inside bucket 0
#   1048681  p3 (257,)         small, bucket boundary 0|1 falls inside it
#   1048938  p4 (1537, 1601)   spans buckets 1, 2, 3            (SPAN)
#   3509675  p5 (31, 33)       small, wholly inside bucket 3
#   3510698  p6 (4, 9)         small, wholly inside bucket 3
#   3510734  p7 (999, 2003)    buckets 3, 4, 5
#   5511731  p8 (1830001,)     buckets 5, 6
#   7341732  p9 (1,)           last 1-element parameter         (LAST)
SHAPES = [(1,), (1023, 1025), (3, 5, 7), (257,), (1537, 1601), (31, 33),
          (4, 9), (999, 2003), (1830001,), (1,)]
SPAN = 4
LAST = len(SHAPES) - 1
SMALL_NUMEL = 4096


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


NUMELS = [_numel(s) for s in SHAPES]
OFFSETS = [sum(NUMELS[:i]) for i in range(len(SHAPES))]
TOTAL = sum(NUMELS)


def bucket_layout(total: int, world: int, zero: bool, n_buckets: int):
    """(padded, [(offset, numel)]) of the documented bucketing: ZeRO cuts the
    shard into n_buckets ranges and a bucket is world x one range; ddp cuts
    the unpadded buffer and holds at most one bucket per 2**20 elements."""
    if zero and world > 1:
        S = (total + world - 1) // world
        nb = max(1, min(n_buckets, S))
        cuts = [S * i // nb for i in range(nb + 1)]
        return S * world, [(cuts[i] * world, (cuts[i + 1] - cuts[i]) * world)
                           for i in range(nb)]
    nb = max(1, min(n_buckets, max(1, total // (1 << 20))))
    cuts = [total * i // nb for i in range(nb + 1)]
    return total, [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(nb)]


def param_buckets(buckets):
    """For every toy parameter, the buckets its flat range overlaps."""
    return [[b for b, (ob, nb_) in enumerate(buckets)
             if o < ob + nb_ and o + n > ob]
            for o, n in zip(OFFSETS, NUMELS)]


def assert_layout(buckets):
    """The properties the toy exists for, at a 7-bucket layout."""
    assert len(buckets) == 7, len(buckets)
    pb = param_buckets(buckets)
    assert len(pb[SPAN]) >= 3, pb[SPAN]
    inner = [ob for ob, _ in buckets[1:]
             if any(o < ob < o + n for o, n in zip(OFFSETS, NUMELS))]
    assert inner, "no bucket boundary strictly inside a parameter"
    small_in = [sum(1 for o, n in zip(OFFSETS, NUMELS)
                    if n <= SMALL_NUMEL and ob <= o and o + n <= ob + nb_)
                for ob, nb_ in buckets]
    assert max(small_in) >= 2, small_in


class Toy(nn.Module):
    def __init__(self, device="cpu", seed: int = 0):
        super().__init__()
        assert TOTAL % 2 == 1 and TOTAL >= 7 * 2 ** 20, TOTAL
        assert NUMELS[0] == 1 and NUMELS[LAST] == 1
        assert_layout(bucket_layout(TOTAL, 1, False, 7)[1])
        padded, zb = bucket_layout(TOTAL, 2, True, 7)
        assert padded == TOTAL + 1
        assert_layout(zb)
        self.ps = nn.ParameterList(
            [nn.Parameter(w.to(device, copy=True)) for w in _toy_init(seed)])


@functools.lru_cache(maxsize=2)
def _toy_init(seed: int):
    g = torch.Generator().manual_seed(1000 + seed)
    return tuple((torch.randn(s, generator=g) * 0.05).to(BF) for s in SHAPES)


# ---------------------------------------------------------------------------
# scripted gradients
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _c_cpu(s: int, k: int, r: int) -> torch.Tensor:
    """Flat bf16 constants of every parameter for (step, microstep, rank):
    randint(-8, 9) / 8 from a CPU generator seeded by (s, k, r, i)."""
    out = torch.empty(TOTAL, dtype=torch.int8)
    for i, (o, n) in enumerate(zip(OFFSETS, NUMELS)):
        g = torch.Generator().manual_seed(((s * 8 + k) * 8 + r) * 64 + i + 7)
        out[o:o + n] = torch.randint(-8, 9, (n,), generator=g, dtype=torch.int8)
    return (out.to(torch.float32) / 8).to(BF)


_C_DEV: dict = {}


def _c_dev(s, k, r, device) -> torch.Tensor:
    device = torch.device(device)
    if device.type == "cpu":
        return _c_cpu(s, k, r)
    key = (s, k, r, str(device))
    if key not in _C_DEV:
        _C_DEV[key] = _c_cpu(s, k, r).to(device)
    return _C_DEV[key]


class Script:
    def __init__(self, K: int, world: int = 1, presence: str = "all",
                 order: str = "forward"):
        assert 1 <= K <= 3 and world in (1, 2)
        assert presence in ("all", "missing") and order in ("forward", "reversed")
        assert presence == "all" or K == 3
        self.K, self.world, self.presence, self.order = K, world, presence, order

    def present(self, k: int, i: int) -> bool:
        """The same on every rank: the launch order cannot differ."""
        if self.presence == "missing":
            if k == 1 and i == SPAN:
                return False
            if k == 2 and i == LAST:
                return False
        return True

    def preload(self, steps, rank: int, device):
        """Put the constants of these steps on the device ahead of time, so
        that the loop itself issues no host-to-device copy."""
        for s in steps:
            for k in range(self.K):
                _c_dev(s, k, rank, device)

    def loss(self, params, s: int, k: int, rank: int) -> torch.Tensor:
        c = _c_dev(s, k, rank, params[0].device)
        idx = [i for i in range(len(SHAPES)) if self.present(k, i)]
        if self.order == "reversed":
            idx.reverse()
        total = None
        for i in idx:
            o, n = OFFSETS[i], NUMELS[i]
            t = (params[i] * c[o:o + n].view(SHAPES[i])).sum()
            total = t if total is None else total + t
        return total

    def expected_full(self, s: int) -> torch.Tensor:
        """fp32 (TOTAL,) sum over microsteps and ranks of the constants of the
        parameters present. Sums of at most 6 multiples of 1/8 in [-1, 1]:
        exact, whatever the order."""
        return _expected_full(s, self.K, self.world, self.presence)


@functools.lru_cache(maxsize=16)
def _expected_full(s, K, world, presence):
    script = Script(K, world, presence)
    acc = torch.zeros(TOTAL, dtype=torch.int32)          # in units of 1/8
    for k in range(K):
        for r in range(world):
            c8 = (_c_cpu(s, k, r).float() * 8).to(torch.int32)
            for i, (o, n) in enumerate(zip(OFFSETS, NUMELS)):
                if script.present(k, i):
                    acc[o:o + n] += c8[o:o + n]
    assert int(acc.abs().max()) < 64
    return acc.float() / 8


# ---------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------
def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def all_zero(t: torch.Tensor) -> bool:
    return int(torch.count_nonzero(t)) == 0


def take_shard(full: torch.Tensor, pieces) -> torch.Tensor:
    """shard[po:po+n] = full[fo:fo+n] for every piece (fo, n, po)."""
    size = sum(n for _, n, _ in pieces)
    out = torch.empty(size, dtype=full.dtype, device=full.device)
    for fo, n, po in pieces:
        out[po:po + n] = full[fo:fo + n]
    return out


def assemble(shards, pieces_per_rank, padded: int) -> torch.Tensor:
    """The full buffer from every rank's shard and piece map; the pieces
    must tile [0, padded) exactly once."""
    full = torch.zeros(padded, dtype=shards[0].dtype, device=shards[0].device)
    cover = torch.zeros(padded, dtype=torch.int32, device=shards[0].device)
    for shard, pieces in zip(shards, pieces_per_rank):
        assert sum(n for _, n, _ in pieces) == shard.numel()
        for fo, n, po in pieces:
            full[fo:fo + n] = shard[po:po + n]
            cover[fo:fo + n] += 1
    assert bool((cover == 1).all()), "piece map does not tile the flat buffer"
    return full


def check_weight_image(flat_w, full_master, total: int):
    assert bits_equal(flat_w[:total], full_master[:total].to(flat_w.dtype)), \
        "flat_w differs from the assembled master"
    assert all_zero(flat_w[total:]), "padded tail of flat_w is not zero"


def check_alias(engine):
    """p.data and p.grad are the views at the parameter's meta offset."""
    w, g = engine.flat_w, engine.flat_g
    for p, (name, shape, o, n) in zip(engine.params, engine.meta):
        assert p.data.data_ptr() == w.data_ptr() + o * w.element_size(), name
        assert p.grad is not None and \
            p.grad.data_ptr() == g.data_ptr() + o * g.element_size(), name
        assert tuple(p.grad.shape) == shape and p.grad.is_contiguous(), name


def make_hp(engine, K: int) -> dict:
    return dict(lr=LR, beta1=engine.beta1, beta2=engine.beta2, eps=engine.eps,
                wd_over_peak_lr=engine.wd_over_peak,
                grad_scale=1.0 / (K * engine.world), clip_norm=engine.grad_clip)


def check_step(engine, before, expected_g, sq, hp, full_g=None, tag="engine"):
    """One optimizer step. ``before``: clones of (master, m, v) taken just
    before engine.step(); ``expected_g``: this rank's exact expected g32 in
    the shard's concatenated piece order; ``sq``: what step() returned;
    ``full_g``: the expected gradient of the whole buffer (default: the shard
    is the whole buffer). Returns the figures it printed."""
    dev = engine.master.device
    expected_g = expected_g.to(dev)
    full_g = expected_g if full_g is None else full_g.to(dev)
    master0, m0, v0 = before
    hp = dict(hp, step=engine.step_count)
    figs = U.adamw_figures((master0, expected_g, m0, v0), sq, hp,
                           (engine.master, engine.m, engine.v))
    U.check(tag, figs)
    # fp32 sum of n non-negative terms: relative error <= ~sqrt(n) 2^-24 =
    # 1.6e-4 even fully sequential; one bucket of one rank-microbatch is 1/42.
    sq_ref = float(full_g.double().pow(2).sum())
    sq_rel = abs(float(sq) - sq_ref) / sq_ref
    print(f"EDGE {tag} sq: got={float(sq):.9e} ref={sq_ref:.9e} rel={sq_rel:.3e} bound=1.000e-03")
    assert sq_rel <= 1e-3, (tag, float(sq), sq_ref)

    assert all_zero(engine.g32), "g32 not zero after the step"
    for i, fg in enumerate(engine.flat_gs):
        assert all_zero(fg), f"flat grad buffer {i} not zero after the step"
    total = engine.total
    for fo, n, po in engine.pieces:
        # weight image of this rank's pieces; the parent repeats it on the
        # master assembled from all ranks
        assert bits_equal(engine.flat_w[fo:fo + n],
                          engine.master[po:po + n].to(engine.flat_w.dtype)), \
            f"flat_w[{fo}:{fo + n}] differs from the master piece"
        if fo + n > total:
            lo = po + max(0, total - fo)
            for name in ("master", "m", "v"):
                assert all_zero(getattr(engine, name)[lo:po + n]), \
                    f"padded tail of {name} is not zero"
    assert all_zero(engine.flat_w[total:]), "padded tail of flat_w is not zero"
    if not engine.zero:
        full = assemble([engine.master], [engine.pieces], engine.padded)
        check_weight_image(engine.flat_w, full, total)
    check_alias(engine)
    return {"figs": [str(f) for f in figs], "sq_rel": sq_rel}


# ---------------------------------------------------------------------------
# launch record
# ---------------------------------------------------------------------------
class Recorder:
    """Wraps engine._launch_bucket on the instance and adds a recording hook
    to every parameter. ``ms`` and ``phase`` are set by run_steps."""

    def __init__(self, engine):
        self.launches = []   # (microstep, bucket, phase)
        self.hooks = []      # (microstep, parameter index)
        self.ms = 0
        self.phase = "backward"
        inner = engine._launch_bucket

        def launch(b):
            self.launches.append((self.ms, b, self.phase))
            return inner(b)

        engine._launch_bucket = launch
        for i, p in enumerate(engine.params):
            p.register_post_accumulate_grad_hook(
                lambda _p, i=i: self.hooks.append((self.ms, i)))

    def of(self, ms: int):
        return [(b, ph) for m, b, ph in self.launches if m == ms]

    def hooks_of(self, ms: int):
        return [i for m, i in self.hooks if m == ms]


def check_launches(rec: Recorder, engine, script: Script, n_micro: int):
    """What the design promises of the launch record of ``n_micro``
    microsteps (microstep t ran script microstep t % K)."""
    nb = engine.n_buckets
    pb = param_buckets(engine.buckets)
    for t in range(n_micro):
        k = t % script.K
        got = rec.of(t)
        assert [b for b, _ in got] == list(range(nb - 1, -1, -1)), (t, got)
        present = [i for i in range(len(SHAPES)) if script.present(k, i)]
        fired = rec.hooks_of(t)
        want = present[::-1] if script.order == "forward" else present
        assert fired == want, (t, fired, want)
        if not engine._hooks_on:
            assert all(ph == "microstep_end" for _, ph in got), (t, got)
            continue
        absent = [i for i in range(len(SHAPES)) if not script.present(k, i)]
        if not absent:
            assert all(ph == "backward" for _, ph in got), (t, got)
        else:
            top = max(b for i in absent for b in pb[i])
            for b, ph in got:
                assert ph == ("microstep_end" if b <= top else "backward"), (t, got)


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
def state_clones(engine):
    return (engine.master.clone(), engine.m.clone(), engine.v.clone())


def shard_of(engine, full_g: torch.Tensor) -> torch.Tensor:
    """This rank's part of a full expected vector, zero-padded."""
    padded = torch.zeros(engine.padded, dtype=full_g.dtype)
    padded[:engine.total] = full_g
    return take_shard(padded, engine.pieces)


def run_steps(engine, toy, script: Script, steps, rank: int = 0, rec=None,
              tag: str = "engine", check: bool = True, errors=None):
    """Run the scripted steps ``steps`` (an iterable of step numbers) with
    check_step after each. A failed check raises, or with ``errors`` (a list)
    is appended to it so that a rank of a pair keeps its collectives in
    lockstep with the other. Returns the per-step figures."""
    params = list(toy.ps)
    hp = make_hp(engine, script.K)
    out = []
    prev = None

    def guarded(fn):
        if errors is None:
            return fn()
        try:
            return fn()
        except AssertionError as e:
            errors.append(f"{tag}: {e}")
            return None

    for s in steps:
        for k in range(script.K):
            guarded(lambda: check_alias(engine))
            if rec is not None:
                rec.phase = "backward"
            script.loss(params, s, k, rank).backward()
            guarded(lambda: check_alias(engine))
            if rec is not None:
                rec.phase = "microstep_end"
            engine.microstep_end()
            if rec is not None:
                rec.ms += 1
        if not check:
            engine.step(LR, script.K)
            continue
        full_g = script.expected_full(s)
        exp_g = shard_of(engine, full_g)
        if not engine._overlap:
            # synchronous path: the accumulator is complete here
            guarded(lambda: _assert(bits_equal(engine.g32, exp_g.to(engine.g32.device)),
                                    f"step {s}: g32 differs from the exact expectation"))
        before = state_clones(engine)
        if prev is not None:
            guarded(lambda: _assert(all(bits_equal(a, b) for a, b in zip(before, prev)),
                                    f"step {s}: state changed between steps"))
        sq = engine.step(LR, script.K)
        r = guarded(lambda: check_step(engine, before, exp_g, sq, hp, full_g=full_g,
                                       tag=f"{tag} step{s}"))
        out.append(r)
        prev = state_clones(engine)
    return out


def _assert(cond, msg):
    assert cond, msg


# ---------------------------------------------------------------------------
# a pair of ranks over gloo (CPU, or both on cuda:0)
# ---------------------------------------------------------------------------
JOIN_TIMEOUT = 240


def scenario_name(zero, nb, clip):
    return f"{'zero' if zero else 'ddp'}_nb{nb}_clip{clip:g}"


def pair_worker(rank, init_file, outdir, scenarios, device, record):
    """One rank of a pair: every scenario in turn, check_step locally, the
    state to ``outdir`` as numpy arrays. A failed check is recorded and the
    run goes on, so that the other rank is never left in a collective."""
    import torch.distributed as dist
    os.environ["WORLD_SIZE"] = "2"
    os.environ["RANK"] = str(rank)
    dist.init_process_group("gloo", init_method=f"file://{init_file}",
                            rank=rank, world_size=2,
                            timeout=datetime.timedelta(seconds=120))
    errors = []
    arrays = {}
    try:
        for zero, nb, clip in scenarios:
            name = scenario_name(zero, nb, clip)
            toy = Toy(device=device)
            engine = ShardedAdamW(toy, compute_dtype=BF, zero=zero, n_buckets=nb,
                                  grad_clip=clip)
            if engine.zero != zero or engine.n_buckets != nb or \
                    engine.buckets != bucket_layout(TOTAL, 2, zero, nb)[1]:
                errors.append(f"{name}: unexpected bucket layout")
            script = Script(3, 2, "missing", "forward")
            script.preload(range(3), rank, device)
            rec = Recorder(engine) if record else None
            run_steps(engine, toy, script, range(3), rank=rank, rec=rec,
                      tag=f"{device} w2 r{rank} {name}", errors=errors)
            if rec is not None:
                try:
                    check_launches(rec, engine, script, 9)
                except AssertionError as e:
                    errors.append(f"{name}: launch record: {e}")
                arrays[f"{name}.launches"] = np.array(
                    [(m, b, ph == "backward") for m, b, ph in rec.launches], dtype=np.int64)
                arrays[f"{name}.hooks"] = np.array(rec.hooks, dtype=np.int64)
            for k in ("master", "m", "v"):
                arrays[f"{name}.{k}"] = getattr(engine, k).cpu().numpy().copy()
            arrays[f"{name}.pieces"] = np.array(engine.pieces, dtype=np.int64)
            arrays[f"{name}.flat_w"] = engine.flat_w.cpu().view(torch.int16).numpy().copy()
    except Exception:
        errors.append(traceback.format_exc())
    arrays["errors"] = np.array(errors, dtype=str)
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), **arrays)
    dist.destroy_process_group()


def run_pair(tmp_path, scenarios, device, record):
    """Spawn the two ranks and wait with a timeout; a rank still running
    then is terminated. Returns (ranks that were stuck, exit codes)."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    init_file = str(tmp_path / "pg_init")
    procs = [ctx.Process(target=pair_worker,
                         args=(r, init_file, str(tmp_path), scenarios, device, record))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=JOIN_TIMEOUT)
    stuck = [p for p in procs if p.is_alive()]
    for p in stuck:
        p.terminate()
        p.join(timeout=10)
    codes = [p.exitcode for p in procs]
    return stuck, codes


def check_pair(tmp_path, scenarios):
    """The parent's view: both ranks' shards assembled by their piece maps."""
    res = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    for r in range(2):
        assert res[r]["errors"].size == 0, "\n".join(res[r]["errors"].tolist())
    for zero, nb, clip in scenarios:
        name = scenario_name(zero, nb, clip)
        padded = bucket_layout(TOTAL, 2, zero, nb)[0]
        fw = [torch.from_numpy(res[r][f"{name}.flat_w"]).view(BF) for r in range(2)]
        assert fw[0].numel() == padded
        assert bits_equal(fw[0], fw[1]), f"{name}: flat_w differs between the ranks"
        pieces = [res[r][f"{name}.pieces"].tolist() for r in range(2)]
        for k in ("master", "m", "v"):
            sh = [torch.from_numpy(res[r][f"{name}.{k}"]) for r in range(2)]
            if zero:
                full = assemble(sh, pieces, padded)
                assert all_zero(full[TOTAL:]), f"{name}: padded tail of {k}"
            else:
                assert bits_equal(sh[0], sh[1]), f"{name}: replicas of {k} differ"
                full = assemble(sh[:1], pieces[:1], padded)
            if k == "master":
                check_weight_image(fw[0], full, TOTAL)
        if f"{name}.launches" in res[0]:
            for k in ("launches", "hooks"):
                assert np.array_equal(res[0][f"{name}.{k}"], res[1][f"{name}.{k}"]), \
                    f"{name}: {k} differ between the ranks"
    return res
