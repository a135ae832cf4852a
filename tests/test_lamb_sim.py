"""The PRODUCT's step schedule with tfa.optimizers.LAMB on it (trainer.py:37-38), on the simulated runtime: Trainer(optimizer=LAMB())
runs LAMB bucket by bucket on the optimizer stream while the backward pass continues, race-checked, and two steps equal the fp64
restatement (tests/lamb_ref.py) applied, Keras variable by Keras variable, to the oracle's gradients - the oracle's variables carry
no padding, so this also holds the norms to the variable's own elements."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LR, N_STEPS = 1e-3, 2


def _oracle_lamb_steps(SS, B, n_steps, opt, kind="unet", world=1):
    """The oracle's gradients (world > 1: per-replica gradients of the global batch's shards, summed), lamb_ref's step.  Returns the parameters, the losses, per variable the distance it can have moved
    (sum over the steps of lr r max|u|) and the names of the variables whose exact gradient is zero."""
    import lamb_ref
    from oracle import torch_ref as R
    cfg, params, loss_and_grads = SS._oracle(kind)
    names = list(params)
    w = {k: torch.tensor(np.asarray(params[k], np.float64)) for k in names}
    m = {k: torch.zeros_like(w[k]) for k in names}
    v = {k: torch.zeros_like(w[k]) for k in names}
    spec_in, emb, spec_out = R.synthetic_batch(R.Config(SS.H, SS.W), B * world)
    losses, moved, dead = [], {k: 0.0 for k in names}, set()
    for t in range(1, n_steps + 1):
        loss, g = 0.0, None
        for r in range(world):
            sl = slice(r * B, (r + 1) * B)
            l, _, _, gr = loss_and_grads({k: w[k].numpy() for k in names}, spec_in[sl], emb[sl], spec_out[sl], B * world, world)
            loss += l
            g = gr if g is None else {k: g[k] + gr[k] for k in gr}
        losses.append(loss)
        # a bias in front of a BatchNorm has the exact gradient 0: what the oracle holds there is fp64 rounding noise, 1e-6 of the largest
        # gradient entry at the very most (the floor of test_schedule_sim), and LAMB's ratio scales that noise to a full step
        gmax = {k: float(torch.as_tensor(g[k]).abs().max()) for k in names}
        floor = 1e-6 * max(gmax.values())
        dead |= {k for k in names if gmax[k] <= floor}
        out = lamb_ref.step([(w[k], torch.as_tensor(g[k]).double(), m[k], v[k], (opt.decayed(k), opt.adapted(k))) for k in names],
                            opt.learning_rate, opt.beta_1, opt.beta_2, opt.epsilon, opt.weight_decay, t=t)
        for k, o in zip(names, out):
            w[k], m[k], v[k] = o["w"], o["m"], o["v"]
            moved[k] += opt.learning_rate * o["r"] * float(o["u"].abs().max())
    return {k: w[k].numpy() for k in names}, losses, moved, dead


@pytest.mark.parametrize("kind", ["unet", "ae"])
def test_lamb_on_the_product_schedule(monkeypatch, kind):
    import lamb_cpu_ops
    import test_schedule_sim as SS
    import unet_rir_amd as U
    from sim_runtime import SimRuntime
    from oracle import torch_ref as R
    rt = SimRuntime()
    impl = lamb_cpu_ops.install(monkeypatch, rt)
    B = 2
    cfg, eng, _ = SS._build(rt, B, True, bucket_bytes=8192, kind=kind)
    opt = U.LAMB(learning_rate=LR)
    tr = U.Trainer(eng, optimizer=opt, dropout=False, bucket_bytes=8192)
    assert eng.optimizer == "lamb" and tr.lr == LR and tr.adam_stream is not None
    spec_in, emb, spec_out = (torch.tensor(a) for a in R.synthetic_batch(cfg, B))
    w0 = eng.export_keras_params()
    want_p, want_l, moved, dead = _oracle_lamb_steps(SS, B, N_STEPS, opt, kind)
    losses = [tr.step(spec_in, emb, spec_out, return_loss=True) for _ in range(N_STEPS)]
    np.testing.assert_allclose(np.array(losses), np.array(want_l), rtol=1e-5)
    # as test_schedule_sim: a near-zero gradient entry's fp32 rounding shows up as a fraction of the step, so every parameter is held to
    # 2 % of the distance it can have moved - for LAMB lr r max|u| per step, taken from the restatement.  A variable whose exact
    # gradient is zero moves along rounding noise, in the product as in the reference, by the length the trust ratio fixes:
    # ||dw|| = lr ||w|| per step.  There the direction is nobody's to predict and the length is what is held.
    got = eng.export_keras_params()
    assert all(n.endswith("bias") for n in dead) and len(dead) < len(want_p) // 3
    for n, w in want_p.items():
        if n in dead:
            step_len = float((got[n].double() - w0[n].double()).norm())
            assert step_len <= N_STEPS * LR * (1 + LR) ** N_STEPS * float(w0[n].double().norm()) * (1 + 1e-5), (n, step_len)
            continue
        err = float(np.abs(got[n].double().numpy() - w).max())
        assert err <= 0.02 * moved[n], (n, err, moved[n])
    # bucket by bucket on the optimizer stream, ordered by events alone; every call a range of whole variables, every variable once per step
    (table,) = impl.lamb_ops.tables
    assert len(tr.bucketer.bounds) > 3 and len(table.calls) == N_STEPS * len(tr.bucketer.bounds) and rt.n_cross_stream > 50
    per_step = table.calls[:len(tr.bucketer.bounds)]
    assert per_step[0][0] == 0 and per_step[-1][1] == eng.theta.numel() and all(a[1] == b[0] for a, b in zip(per_step, per_step[1:]))
    # padded channels and alignment tails stay exactly zero
    for n, s_ in eng.specs.items():
        assert float(eng.theta[s_.offset + s_.numel:s_.end].abs().max() if s_.end > s_.offset + s_.numel else 0.0) == 0.0, n
        if s_.kind in ("conv_padin", "convT_padout"):
            assert float(eng.p[n][..., 2:].abs().max()) == 0.0, n
        if s_.kind in ("conv_padout", "bias_pad"):
            assert float(eng.p[n][2:].abs().max()) == 0.0, n


def test_lamb_selection_and_misuse(monkeypatch):
    import lamb_cpu_ops
    import test_schedule_sim as SS
    import unet_rir_amd as U
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    lamb_cpu_ops.install(monkeypatch, rt)
    _, eng, tr0 = SS._build(rt, 2, False)
    assert eng.optimizer == "adam" and tr0.lr == 1e-3
    with pytest.raises(ValueError, match="unet_rir_amd.LAMB"):
        U.Trainer(eng, optimizer="lamb")                               # the name stays refused: LAMB is selected by an object
    opt = U.LAMB(weight_decay=0.01, exclude_from_weight_decay=["bias", r"\.gamma$", r"\.beta$"])
    assert (opt.learning_rate, opt.beta_1, opt.beta_2, opt.epsilon) == (0.001, 0.9, 0.999, 1e-6)
    assert opt.exclude_from_layer_adaptation == opt.exclude_from_weight_decay         # tfa: falls back to the weight-decay list
    tr = U.Trainer(eng, optimizer=opt, lr=5e-4, graph=True)
    assert eng.optimizer == "lamb" and tr.lr == 5e-4 and tr.use_graph
    assert U.Trainer(eng, optimizer=opt).lr == 0.001 and not U.Trainer(eng, optimizer="nadam", graph=True).use_graph
    eng.set_lamb(opt)
    table = eng._lamb_table()
    names = list(eng.specs)
    for (off, cnt, slot, dec, ada), n in zip(table.segments, names):
        s_ = eng.specs[n]
        assert (off, cnt, slot) == (s_.offset, s_.numel, s_.end - s_.offset)
        assert dec == ada == (not ("bias" in n or n.endswith(".gamma") or n.endswith(".beta"))), n
    assert any(not s[3] for s in table.segments) and any(s[3] for s in table.segments)
    assert eng._lamb_table() is table                                  # built once per parameter set
    args = eng.adam_begin(1e-3)
    big = next(s_ for s_ in eng.specs.values() if s_.end - s_.offset >= 128)
    eng.adam_range(big.offset, big.end, *args)                         # a whole variable: fine
    for lo, hi in ((big.offset + 64, big.end), (big.offset, big.end - 64), (big.end, big.end), (big.end, big.offset)):
        with pytest.raises(ValueError):
            eng.adam_range(lo, hi, *args)


def _dp_worker(rank, world, port, out_path, B=2):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import lamb_cpu_ops
        import test_schedule_sim as SS
        import unet_rir_amd as U
        from sim_runtime import SimRuntime
        from oracle import torch_ref as R
        mpatch = pytest.MonkeyPatch()
        rt = SimRuntime()
        lamb_cpu_ops.install(mpatch, rt)
        cfg, eng, _ = SS._build(rt, B, True, world=world, bucket_bytes=8192)
        tr = U.Trainer(eng, optimizer=U.LAMB(learning_rate=LR), dropout=False, world_size=world, bucket_bytes=8192)
        tr.broadcast_parameters(0)
        spec_in, emb, spec_out = R.synthetic_batch(cfg, B * world)
        sl = slice(rank * B, (rank + 1) * B)
        t = torch.tensor
        losses = [tr.step(t(spec_in[sl]), t(emb[sl]), t(spec_out[sl]), return_loss=True) for _ in range(N_STEPS)]
        lt = torch.tensor(losses, dtype=torch.float64)
        dist.all_reduce(lt)
        torch.save({"params": {k: v.double() for k, v in eng.export_keras_params().items()}, "losses": lt, "theta": eng.theta.clone(),
                    "n_all_reduce": len(rt.collectives), "n_buckets": len(tr.bucketer.bounds)}, f"{out_path}.{rank}")
        mpatch.undo()
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_run_lamb_on_the_all_reduced_gradient_and_stay_bit_identical(tmp_path):
    """Data parallel (MirroredStrategy semantics as test_schedule_sim): each bucket's LAMB launch waits for that bucket's SUM
    all-reduce, so every rank forms the same norms from the same summed gradient - the ranks end bit-identical and equal the
    restatement applied to the summed per-replica gradients of the oracle."""
    import test_schedule_sim as SS
    import unet_rir_amd as U
    world = 2
    out = str(tmp_path / "dp")
    mp.spawn(_dp_worker, args=(world, 32700 + (os.getpid() % 1500), out), nprocs=world, join=True)
    want_p, want_l, moved, dead = _oracle_lamb_steps(SS, 2, N_STEPS, U.LAMB(learning_rate=LR), "unet", world)
    res = [torch.load(f"{out}.{r}") for r in range(world)]
    assert torch.equal(res[0]["theta"], res[1]["theta"])
    for r in range(world):
        assert res[r]["n_buckets"] > 3 and res[r]["n_all_reduce"] == N_STEPS * res[r]["n_buckets"]
        np.testing.assert_allclose(res[r]["losses"].numpy(), np.array(want_l), rtol=1e-5)
        for n, w in want_p.items():
            if n not in dead:
                err = float(np.abs(res[r]["params"][n].numpy() - w).max())
                assert err <= 0.02 * moved[n], (r, n, err, moved[n])
