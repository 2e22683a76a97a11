"""Exact checks of the training engine's overlap pipeline on the GPU: double
flat grad buffers, bucket launches from backward hooks on the side stream,
deferred fp32 accumulation, the ZeRO piece map and weight all-gather, and the
event that gates the async checkpoint snapshot.

The scripted-gradient toy of engine_util gives the accumulated gradient one
right value per element (see there), so a bucket reduced before its last grad
landed, a microbatch piece dropped or counted twice, or a weight piece
gathered to the wrong offset cannot hide in a tolerance. The update is held
to the per-element fp64 bound of kernel_edge_util.adamw_figures, the same
bound test_adamw_elements uses. Figures measured on one MI355X are in
profiles/engine_exact.md.
"""
import functools

import pytest
import torch

import engine_util as E

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from midgpt_amd import ops
    assert ops.have_ext()

from midgpt_amd.config import GPTConfig
from midgpt_amd.data import synthetic_batch
from midgpt_amd.models.gpt import GPT
from midgpt_amd.parallel.engine import ShardedAdamW

DEV = "cuda"

# (n_buckets, K, clip, order, presence): every value of every axis at least
# once, each n_buckets with both orders and both presence patterns.
COMBOS = [
    (1, 1, 1.0, "forward", "all"),
    (1, 3, 1e30, "reversed", "missing"),
    (4, 3, 1.0, "forward", "all"),
    (4, 3, 1e30, "forward", "missing"),
    (4, 1, 1e30, "reversed", "all"),
    (7, 3, 1.0, "forward", "missing"),
    (7, 3, 1e30, "reversed", "all"),
    (7, 1, 1.0, "forward", "all"),
    (7, 3, 1.0, "reversed", "missing"),
]


def _engine(n_buckets, clip=1.0, seed=0):
    toy = E.Toy(device=DEV, seed=seed)
    engine = ShardedAdamW(toy, compute_dtype=E.BF, zero=True,
                          grad_clip=clip, n_buckets=n_buckets)
    assert engine._overlap and not engine.zero
    assert engine.n_buckets == n_buckets
    assert engine._hooks_on == (n_buckets > 1)
    assert engine.buckets == E.bucket_layout(E.TOTAL, 1, False, n_buckets)[1]
    return toy, engine


# ---------------------------------------------------------------------------
# 1. world 1, overlap pipeline
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_buckets,K,clip,order,presence", COMBOS)
def test_world1_overlap_exact(n_buckets, K, clip, order, presence):
    toy, engine = _engine(n_buckets, clip)
    script = E.Script(K, 1, presence, order)
    script.preload(range(3), 0, DEV)
    rec = E.Recorder(engine)
    out = E.run_steps(engine, toy, script, range(3), rec=rec,
                      tag=f"gpu w1 nb{n_buckets} K{K} clip{clip:g} {order} {presence}")
    assert len(out) == 3 and engine.step_count == 3
    E.check_launches(rec, engine, script, 3 * K)


# ---------------------------------------------------------------------------
# 2. launch record
# ---------------------------------------------------------------------------
def _record(n_buckets, order, presence):
    toy, engine = _engine(n_buckets)
    script = E.Script(3, 1, presence, order)
    script.preload(range(1), 0, DEV)
    rec = E.Recorder(engine)
    E.run_steps(engine, toy, script, range(1), rec=rec, check=False)
    torch.cuda.synchronize()
    E.check_launches(rec, engine, script, 3)
    print(f"EDGE launch record nb{n_buckets} {order} {presence}: "
          f"launches={rec.launches} hooks={rec.hooks}")
    return rec


@pytest.mark.parametrize("n_buckets", [4, 7])
def test_launch_record(n_buckets):
    nb = n_buckets
    n_par = len(E.SHAPES)
    fwd = _record(nb, "forward", "all")
    rev = _record(nb, "reversed", "all")
    down = list(range(nb - 1, -1, -1))
    for t in range(3):
        # the overlap the design claims: every bucket goes out from a hook
        assert fwd.of(t) == [(b, "backward") for b in down]
        assert fwd.hooks_of(t) == list(range(n_par - 1, -1, -1))
        # "reversed" really is the opposite hook order, and the launches
        # still go out descending (all from the last hook that fires)
        assert rev.hooks_of(t) == fwd.hooks_of(t)[::-1]
        assert [b for b, _ in rev.of(t)] == down
    miss = _record(nb, "forward", "missing")
    pb = E.param_buckets(E.bucket_layout(E.TOTAL, 1, False, nb)[1])
    assert miss.of(0) == [(b, "backward") for b in down]
    # microstep 2 lacks the parameter that spans three buckets: the buckets
    # above it go out from hooks, its own and all lower ones at the end
    top = max(pb[E.SPAN])
    assert 0 < top < nb - 1
    assert miss.of(1) == [(b, "backward" if b > top else "microstep_end") for b in down]
    # microstep 3 lacks the last parameter: the top bucket never gets ready
    assert miss.of(2) == [(b, "microstep_end") for b in down]
    assert E.LAST not in miss.hooks_of(2) and E.SPAN not in miss.hooks_of(1)


# ---------------------------------------------------------------------------
# 3. world 2 on one GPU (two spawned ranks share cuda:0 over gloo)
# ---------------------------------------------------------------------------
# (zero, n_buckets, clip); clip 1e30 is the one that shows a wrong grad_scale
SCENARIOS_W2 = [(True, 4, 1e30), (True, 7, 1.0), (False, 4, 1e30)]


def test_world2_one_gpu_exact(tmp_path):
    stuck, codes = E.run_pair(tmp_path, SCENARIOS_W2, "cuda:0", record=True)
    if stuck or any(c is None or c < 0 for c in codes):
        # a rank hung or died by a signal: nothing more goes onto this GPU
        pytest.exit(f"two-rank GPU worker hung or crashed (exit codes {codes})",
                    returncode=1)
    assert codes == [0, 0], codes
    res = E.check_pair(tmp_path, SCENARIOS_W2)
    for zero, nb, clip in SCENARIOS_W2:
        name = E.scenario_name(zero, nb, clip)
        la = res[0][f"{name}.launches"]
        assert la.shape == (9 * nb, 3)
        print(f"EDGE launch record w2 {name}: (microstep, bucket, from_hook)="
              f"{la.tolist()}")


# ---------------------------------------------------------------------------
# 4. checkpoint snapshot
# ---------------------------------------------------------------------------
def test_checkpoint_snapshot_is_state_at_save(tmp_path):
    from midgpt_amd.utils import checkpoint as ckpt
    script = E.Script(3, 1, "all", "forward")
    script.preload(range(4), 0, DEV)
    toy_a, eng_a = _engine(4)
    toy_b, eng_b = _engine(4)
    E.run_steps(eng_b, toy_b, script, range(2), check=False)
    E.run_steps(eng_a, toy_a, script, range(2), check=False)
    saved = E.state_clones(eng_a)
    mngr = ckpt.CheckpointManager(str(tmp_path), save_interval=1)
    mngr.save(2, eng_a)
    # no sync: the next steps queue up behind the snapshot
    E.run_steps(eng_a, toy_a, script, range(2, 4), check=False)
    E.run_steps(eng_b, toy_b, script, range(2, 4), check=False)
    mngr.wait()
    state = ckpt.load_full_state(str(tmp_path), 2)
    assert state["step_count"] == 2 and eng_a.step_count == 4
    for name, want in zip(("master", "m", "v"), saved):
        assert E.bits_equal(state[name], want.cpu()), \
            f"{name} on disk is not the state at save()"
    # the gate changes timing only
    for name in ("master", "m", "v"):
        assert E.bits_equal(getattr(eng_a, name), getattr(eng_b, name)), name
    assert E.bits_equal(eng_a.flat_w, eng_b.flat_w)
    assert not E.bits_equal(eng_a.master, saved[0])


# ---------------------------------------------------------------------------
# 5. real model, hooks on versus off
# ---------------------------------------------------------------------------
MID = GPTConfig(block_size=128, vocab_size=512, n_layer=3, n_head=2,
                n_embd=256, dropout=0.0)


@functools.lru_cache(maxsize=None)
def _model_run(n_buckets, rep):
    torch.manual_seed(0)
    model = GPT(MID).to(DEV)
    model.remat = True
    engine = ShardedAdamW(model, compute_dtype=E.BF, zero=False,
                          n_buckets=n_buckets)
    assert engine.total >= 2 * 2 ** 20
    assert engine._hooks_on == (n_buckets > 1)
    assert engine.n_buckets == (1 if n_buckets == 1 else 2)
    g = torch.Generator().manual_seed(11)
    x, y = synthetic_batch(512, 128, 4, 3, device=DEV, generator=g)
    for _ in range(2):
        for k in range(3):
            model.loss(x[k], y[k]).backward()
            engine.microstep_end()
        engine.step(1e-3, 3)
    E.check_alias(engine)
    assert E.bits_equal(engine.flat_w, engine.master.to(E.BF))
    return engine.master.cpu()


def test_model_backward_is_deterministic():
    a, b = _model_run(1, 0), _model_run(1, 1)
    d = float((a - b).abs().max())
    print(f"EDGE model hooks-off run-to-run max |diff| d={d:.3e}")
    assert E.bits_equal(a, b), d


def test_model_hooks_on_equals_hooks_off():
    a, b = _model_run(1, 0), _model_run(1, 1)
    h = _model_run(4, 0)
    d = float((a - b).abs().max())
    dh = max(float((h - a).abs().max()), float((h - b).abs().max()))
    print(f"EDGE model hooks-on vs hooks-off max |diff|={dh:.3e} (d={d:.3e})")
    assert torch.isfinite(h).all()
    if d == 0.0:
        assert E.bits_equal(h, a), dh
    else:
        # the backward itself is not run-to-run exact: allow one more
        # independent draw of the same noise, elementwise
        assert bool(((h - a).abs() <= 4 * d).all()) or \
            bool(((h - b).abs() <= 4 * d).all()), (dh, d)
