"""First-touch weight gradients (round 6): the weight matrices of the gradient arena are not zeroed per step -- their first writer ASSIGNS
(lav_gemm_epilogue.assign / lav_gemm_tn_job.assign / lav_*_bwd_desc.assign_mask), later writers accumulate, and what nobody wrote is zeroed
before anything reads it.  Kernel level: an assigning launch into a poisoned C equals the accumulating launch into a zeroed C, bit for bit, on
every weight-gradient kernel (128 x 128, 256 x 128, ping-pong 256 x 256, split-K through the workspace, grouped launches, a ragged long
contraction).  Model level: three optimizer steps with the mode on and off leave the same parameters (up to the summation order of the atomically accumulated vectors) (agent.py:235-250 semantics:
zero_grad after every step), also with gradient accumulation over two backward passes and for a weight that stops being used."""
import numpy as np
import pytest
import torch

from tests.helpers import BERT_CFGS, Tok, hf_cfg, make_args, make_batch

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16


def rb(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (scale * torch.randn(*shape, device="cuda", generator=g)).to(bf16)


@pytest.mark.parametrize("M,N,Kd,splits", [(768, 768, 8192, 1), (768, 768, 8192, 8), (3072, 768, 4096, 4), (200, 768, 4096, 2), (128, 96, 4096, 1),
                                           (128, 96, 4096, 3), (512, 384, 7840, 4), (768, 768, 30280, 8), (96, 40, 512, 1)])
def test_assigning_weight_gradient_equals_accumulating_into_zero(M, N, Kd, splits):
    from lavender_amd import hip as K
    A, Bm = rb(Kd, M, seed=3), rb(Kd, N, seed=4)
    bias_ref, bias_got = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
    ref = torch.zeros(M, N, device="cuda")
    K.gemm(2, A, Bm, M, N, Kd, out=ref, accumulate=True, splits=splits, rowsum_a=bias_ref)
    got = torch.full((M, N), float("nan"), device="cuda")             # poisoned: an accumulating kernel would keep the NaNs
    K.gemm(2, A, Bm, M, N, Kd, out=got, accumulate=True, splits=splits, rowsum_a=bias_got, assign=True)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert torch.allclose(bias_got, bias_ref, rtol=1e-5, atol=1e-3)          # (the bias gradient is summed with atomics across the splits: order-dependent)
    K.gemm(2, A, Bm, M, N, Kd, out=got, accumulate=True, splits=splits)                   # a second writer accumulates
    K.gemm(2, A, Bm, M, N, Kd, out=ref, accumulate=True, splits=splits)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)


def test_grouped_launch_assigns_per_job():
    from lavender_amd import hip as K
    R_, H, F = 4096, 768, 3072
    ops = [(rb(R_, H, seed=1), rb(R_, F, seed=2)), (rb(R_, F, seed=3), rb(R_, H, seed=4)), (rb(R_, H, seed=5), rb(R_, H, seed=6)), (rb(R_, 3 * H, seed=7), rb(R_, H, seed=8))]
    for gs in (1, 3):
        ref = [torch.zeros(a.shape[1], b.shape[1], device="cuda") for a, b in ops]
        got = [torch.full_like(r, float("nan")) if j != 2 else torch.ones_like(r) for j, r in enumerate(ref)]
        ref[2] += 1.0                                               # job 2 accumulates into existing values, the others assign
        K.gemm_tn_grouped([dict(A=a, B=b, out=o, fallback_splits=2) for (a, b), o in zip(ops, ref)], gs)
        K.gemm_tn_grouped([dict(A=a, B=b, out=o, fallback_splits=2, assign=(j != 2)) for j, ((a, b), o) in enumerate(zip(ops, got))], gs)
        torch.cuda.synchronize()
        for j, (u, v) in enumerate(zip(got, ref)):
            assert torch.equal(u, v), f"grouped launch, splits {gs}, job {j}"


def _micro_agent(first_touch):
    import lavender_amd as LA
    import lavender_amd.arena as AR
    from oracle import lavender_ref as R
    old = AR.FIRST_TOUCH
    AR.FIRST_TOUCH = first_touch
    try:
        cfg = dict(hf_cfg("micro"))
        args = make_args("micro", "micro", 2, txt_backbone=cfg, fusion_encoder=cfg, tokenizer=cfg, lr=1e-3, decay=1e-3, max_iter=100, max_grad_norm=1.0)
        m = LA.LAVENDER_Pretrain_MLM(args, Tok())
        sd = m.state_dict()
        new = {k: R.fill_tensor(k, v.shape) for k, v in sd.items() if v.is_floating_point()}
        new["fc_mtm.predictions.decoder.bias"] = new["fc_mtm.predictions.bias"]
        m.load_state_dict(new, strict=False)
        m.cuda()
        m.arena()                                                   # (built on first use: under the switch)
        ag = LA.Agent_Pretrain_MLM(args, m)
    finally:
        AR.FIRST_TOUCH = old
    assert bool(m.arena().ft_units) == first_touch
    return m, ag


def _batch(ag, step):
    from oracle import lavender_ref as R
    batch = make_batch(2, vocab=BERT_CFGS["micro"]["vocab"], seed=1 + step)
    torch.manual_seed(88 + step)
    batch["txt"], batch["ans_mtm"] = R.masking(batch["txt"])
    np.random.seed(88 + step)
    return ag.prepare_batch(batch)


def _steps(ag, n):
    from lavender_amd import hip as K
    K.reseed(1234)
    for step in range(n):
        ag.step(_batch(ag, step), True)
    torch.cuda.synchronize()


def test_gradient_accumulation_over_two_backward_passes():
    """the second backward pass of a step ACCUMULATES into what the first one assigned (no zero_grad in between)"""
    from lavender_amd import engine as E, hip as K
    grads = []
    for ft in (True, False):
        m, ag = _micro_agent(ft)
        _steps(ag, 1)                                                 # leaves every unit armed (stale memory) in the first-touch model
        K.reseed(99)
        ag._set_mode(True)
        for i in range(2):
            out = ag.forward_step(_batch(ag, 5 + i))
            ls = [ag.loss_func(o.flatten(0, len(o.shape) - 2), a.flatten(0, len(a.shape) - 1)) for o, a in
                  ((out["out_mtm"], out["ans_mtm"]), (out["out_vtm"], out["ans_vtm"]))]
            (ls[0] + ls[1]).backward()
        E.dw_join()
        torch.cuda.synchronize()
        grads.append(m.arena().grad.clone())
    # (vector gradients are summed with float atomics and the two models went through an optimizer step: equal up to summation order, not bits)
    d = (grads[0] - grads[1]).double().norm() / grads[1].double().norm()
    print(f"two-pass gradient arenas: relative difference {float(d):.3e}")
    assert float(d) < 1e-4


def test_full_backward_first_touch_vs_accumulate_on_the_same_parameters():
    """One model, one set of parameters, the same batch and dropout seeds, two backward passes: (i) the shipped mode -- every weight matrix of the
    gradient arena POISONED with NaN and armed, as after zero_grad -- and (ii) the conventional one -- arena zeroed, every unit marked written so
    that all writers accumulate.  The matrices must agree bit for bit (no NaN survives: every one of them was assigned by its first writer), the
    atomically summed vectors up to summation order."""
    from lavender_amd import engine as E, hip as K
    m, ag = _micro_agent(True)
    _steps(ag, 2)                                                     # a trained-for-two-steps state; zero_grad has armed every unit
    ar = m.arena()
    assert ar._ft_armed == len(ar.ft_units) > 20 and all(u.state == 1 for u in ar.ft_units)
    assert all(float(ar.grad[u.lo:u.hi].abs().max()) > 0 for u in ar.ft_units)       # the matrices were NOT zeroed: last step's gradient is still there
    grads = []
    for mode in ("first-touch", "accumulate"):
        if mode == "first-touch":
            for u in ar.ft_units:
                ar.grad[u.lo:u.hi].fill_(float("nan"))
        else:
            ar.grad_full.zero_()
            for u in ar.ft_units:
                u.state = 2
            ar._ft_armed = 0
        K.reseed(4321)
        ag._set_mode(True)
        out = ag.forward_step(_batch(ag, 7))
        ls = [ag.loss_func(o.flatten(0, len(o.shape) - 2), a.flatten(0, len(a.shape) - 1)) for o, a in
              ((out["out_mtm"], out["ans_mtm"]), (out["out_vtm"], out["ans_vtm"]))]
        (ls[0] + ls[1]).backward()
        E.dw_join()
        torch.cuda.synchronize()
        grads.append(ar.grad.clone())
        ar.zero_grad()
    g1, g0 = grads
    assert not bool(torch.isnan(g1).any()), "a poisoned weight gradient was accumulated into, not assigned"
    tied = m.enc_txt.emb_txt.word_embeddings.weight.__dict__["_lav_ft"]      # decoder GEMM (assign) + embedding scatter (float atomics): order-dependent sums
    for u in ar.ft_units:
        if u is tied:
            assert torch.allclose(g1[u.lo:u.hi], g0[u.lo:u.hi], rtol=1e-4, atol=1e-6)
        else:
            assert torch.equal(g1[u.lo:u.hi], g0[u.lo:u.hi]), f"weight gradient at [{u.lo}, {u.hi}) differs between assign and accumulate"
    d = float((g1 - g0).double().norm() / g0.double().norm())
    print(f"whole gradient arena, first-touch vs accumulate: relative difference {d:.3e}")
    assert d < 1e-5


def test_a_weight_nobody_writes_reads_as_zero_not_as_last_steps_gradient():
    """the task head `fc` (main_pretrain_task_specific.py:126-132) is part of the model but not of the MLM step: after a step that DID write
    a unit, a step that does not must leave zeros there before the optimizer / the user reads it"""
    from lavender_amd import engine as E
    m1, a1 = _micro_agent(True)
    ar = m1.arena()
    _steps(a1, 1)
    u = ar.ft_units[0]
    assert u.state == 1                                               # armed by zero_grad: the memory still holds step 1's gradient
    stale = ar.grad[u.lo:u.hi].clone()
    assert float(stale.abs().max()) > 0
    E.dw_join()                                                       # what the end of any backward / the optimizer / a reducer does first
    assert u.state == 0 and float(ar.grad[u.lo:u.hi].abs().max()) == 0.0
    # an accumulating writer (atomics, an un-converted call site) into an ARMED unit zeroes it first
    _steps(a1, 1)
    u = ar.ft_units[1]
    assert u.state == 1
    E.G(next(p for p in m1.parameters() if p.__dict__.get("_lav_ft") is u))
    assert u.state == 2 and float(ar.grad[u.lo:u.hi].abs().max()) == 0.0


def test_a_listener_write_into_a_clean_unit_is_not_read_as_next_steps_gradient():
    """The contract the data-parallel reducer relies on: a listener of the arena (dp.ArenaReducer) may write into a unit after finish_first_touch
    has zeroed it and marked it CLEAN (its all-reduce lands the other ranks' gradient there).  The next step must still read zero where nobody
    writes.  A stub listener plays the reducer on the score head `fc` of LAVENDER_Pretrain, which only the VTM loss writes.  Break caught: zero_grad
    re-arming only the units with a non-zero state."""
    import lavender_amd as LA
    from lavender_amd.engine import dw_join
    args = make_args("micro", "micro", 2, lr=1e-3)
    torch.manual_seed(3)
    m = LA.LAVENDER_Pretrain(args, Tok()).cuda()
    ar = m.arena()
    ag = LA.Agent_Pretrain(args, m)
    u = m.fc[1].weight.__dict__.get("_lav_ft")
    assert u is not None

    def backward(with_vtm):
        b = make_batch(2, vocab=BERT_CFGS["micro"]["vocab"], seed=30)
        torch.manual_seed(50)
        b.update(ag.masking(b["txt"], b["mask"]))
        batch = ag.prepare_batch(b)
        m.eval()
        ar.zero_grad()
        np.random.seed(0)
        out = ag.forward_step((batch["img"], batch["txt"], batch["mask"], batch["ans_mtm"]))
        ls = ag.loss_func(out["out_mtm"].flatten(0, 1), out["ans_mtm"].flatten())
        if with_vtm:
            ls = ls + ag.loss_func(out["out_vtm"], out["ans_vtm"], out["ans_vtm"].shape[0])
        ls.backward()
        dw_join()
        torch.cuda.synchronize()
        return ar.grad[u.lo:u.hi].clone()

    g_fc = backward(True)                                          # no listener yet: the plain gradient of fc
    assert float(g_fc.abs().max()) > 0

    class Stub:
        writes = 0
        events = 0

        def __call__(self, event):
            if event != "fusion_grads_final":
                return
            self.events += 1
            ar.finish_first_touch(u.lo, u.hi)                       # what ArenaReducer._reduce does first
            if self.writes:
                ar.grad[u.lo:u.hi].fill_(3.0)                      # ... and what its all-reduce leaves there: another rank's gradient
                self.writes -= 1

    stub = Stub()
    ar.listeners.append(stub)
    try:
        backward(True)
        stub.writes = 1
        g = backward(False)                                        # fc not written here: zeroed, CLEAN, then written by the listener
        assert stub.events == 2 and u.state == 0 and bool((g == 3.0).all())
        g = backward(False)                                        # nobody writes fc in this step: it must read zero
        assert float(g.abs().max()) == 0.0, f"fc holds {float(g.abs().max())}: the listener's write was carried into the next step"
        g = backward(True)                                         # written again: the plain gradient, nothing added to it
        assert torch.allclose(g, g_fc, rtol=1e-5, atol=0)
    finally:
        ar.listeners.remove(stub)
