"""MI355X: lav_caption_loss_fwd_bwd (label-smoothed loss, drop-the-worst selection, accuracy count, in-place gradient) against the float64 reference
with the error bounds derived in tests/caption_loss_ref.py.  Every check prints measured / bound before it asserts."""
import numpy as np
import pytest
import torch

from tests import caption_loss_ref as CR

pytestmark = pytest.mark.gpu

CONFIGS = [(0.0, 0.0), (0.1, 0.0), (0.1, 0.25), (0.0, 0.25)]          # (label_smoothing, drop_worst_ratio)
SHAPES = {"bert": (30522, 30528, 1.0), "ragged": (1003, 1008, 0.25)}   # V, ld, sigma of the logits (small V: narrow rows keep the loss ladder apart)
N_LAB = {1: 1, 7: 2, 150: 22, 1200: 180}                               # about 15 % labelled; 7 rows take two so that ratio 0.25 keeps one


def _device_buffer(x, ld, pad_value=7.0):
    """(rows, ld) bf16 buffer with x in its first V columns and a non-zero filler in the padding columns, and its (rows, V) view"""
    rows, V = x.shape
    buf = torch.full((rows, ld), pad_value, dtype=torch.bfloat16, device="cuda")
    buf[:, :V] = torch.from_numpy(x).cuda().bfloat16()
    return buf, buf[:, :V]


def _ratio(name, err, bound):
    err, bound = float(err), float(bound)
    print(f"    {name}: measured {err:.3e} bound {bound:.3e} ratio {err / bound if bound > 0 else (0.0 if err == 0 else float('inf')):.3f}")
    return err <= bound


def _run(x, labels, ld, eps, k, select, write_grad=True):
    from lavender_amd import hip as K
    buf, view = _device_buffer(x, ld)
    out, row_loss, correct, kept = K.caption_loss(view, x.shape[1], torch.from_numpy(labels).cuda(), eps, k, select, write_grad)
    torch.cuda.synchronize()
    return buf, out.cpu(), row_loss.cpu(), correct.cpu(), kept.cpu()


@pytest.mark.parametrize("rows", [1, 7, 150, 1200])
@pytest.mark.parametrize("shape", ["bert", "ragged"])
def test_caption_loss_kernel_matches_float64(shape, rows):
    from lavender_amd.captioning import kept_count
    V, ld, sigma = SHAPES[shape]
    n_lab = N_LAB[rows]
    x, labels = CR.make_case(rows, V, n_lab, seed=rows + V, sigma=sigma)
    ok = True
    for eps, ratio in CONFIGS:
        print(f"V {V} ld {ld} rows {rows} labelled {n_lab} eps {eps} ratio {ratio}")
        if ratio > 0 and int(n_lab * (1 - ratio)) == 0:
            with pytest.raises(ValueError, match="mean of no rows"):       # one labelled row: the reference averages nothing (NaN)
                kept_count(n_lab, ratio)
            continue
        k = kept_count(n_lab, ratio) if ratio > 0 else n_lab
        ref = CR.captioning_loss(x, labels, eps, ratio)
        assert ref["k"] == k
        b = CR.bounds(x, labels, eps, ld, ref)
        # the inputs: losses of the labelled rows further apart than their bounds, so the kept set does not depend on rounding
        lab = labels >= 0
        order = np.nonzero(lab)[0][np.argsort(ref["row_loss"].numpy()[lab], kind="stable")]
        if len(order) > 1:
            gap = np.diff(ref["row_loss"].numpy()[order])
            need = b["row_loss"].numpy()[order][1:] + b["row_loss"].numpy()[order][:-1]
            print(f"    smallest loss gap {gap.min():.3e}, bounds of the pair {need[np.argmin(gap)]:.3e}")
            assert (gap > need).all()
        buf, out, row_loss, correct, kept = _run(x, labels, ld, eps, k, select=ratio > 0)
        buf2, out2, row_loss2, correct2, kept2 = _run(x, labels, ld, eps, k, select=ratio > 0)
        assert torch.equal(out, out2) and torch.equal(row_loss, row_loss2) and torch.equal(buf, buf2)      # run-to-run identical bits
        assert torch.equal(correct, correct2) and torch.equal(kept, kept2)
        e_row = (row_loss.double() - ref["row_loss"]).abs()
        worst = int(torch.argmax(e_row / b["row_loss"].clamp_min(1e-300)))
        ok &= _ratio("row loss (worst row)", e_row[worst], b["row_loss"][worst])
        assert (e_row <= b["row_loss"]).all()
        assert (row_loss[~lab] == 0).all()
        assert torch.equal(kept.bool(), ref["kept"]), "kept set"
        assert torch.equal(correct.bool(), ref["correct"]), "correct flags"
        ok &= _ratio("total loss", abs(out[0].item() - ref["total"]), b["total"])
        ok &= _ratio("mean loss", abs(out[0].item() / out[1].item() - ref["loss"]), b["loss"])
        assert out[1].item() == k and out[2].item() == int(ref["correct"].sum()) and out[3].item() == n_lab
        g = buf.float().cpu().double()
        assert (g[:, V:] == 0).all(), "padding columns"
        assert (g[~ref["kept"].numpy()] == 0).all(), "dropped and unlabelled rows"
        e_g = (g[:, :V] - ref["grad"]).abs()
        r_g = e_g / b["grad"].clamp_min(1e-300)
        r_g[b["grad"] == 0] = 0
        i = int(torch.argmax(r_g))
        ok &= _ratio("gradient (worst element)", e_g.flatten()[i], b["grad"].flatten()[i])
        assert (e_g <= b["grad"]).all()
        # evaluation: same results, logits untouched
        buf3, out3, row_loss3, correct3, kept3 = _run(x, labels, ld, eps, k, select=ratio > 0, write_grad=False)
        assert torch.equal(out3, out) and torch.equal(row_loss3, row_loss) and torch.equal(kept3, kept) and torch.equal(correct3, correct)
        assert torch.equal(buf3[:, :V].float().cpu(), torch.from_numpy(x)) and (buf3[:, V:].float() == 7.0).all()
    assert ok


def test_all_rows_unlabelled():
    V, ld = 1003, 1008
    x = CR.make_logits(7, V, seed=11, sigma=0.25)
    labels = np.full(7, -1, dtype=np.int64)
    for select in (False, True):
        buf, out, row_loss, correct, kept = _run(x, labels, ld, 0.1, 0, select)
        assert out.tolist() == [0.0, 0.0, 0.0, 0.0]
        assert (row_loss == 0).all() and (correct == 0).all() and (kept == 0).all()
        assert (buf.float() == 0).all()
        buf, out, *_ = _run(x, labels, ld, 0.1, 0, select, write_grad=False)
        assert torch.equal(buf[:, :V].float().cpu(), torch.from_numpy(x))


def test_ties_keep_the_lower_row_and_argmax_takes_the_lowest_column():
    """equal rows have equal losses: of the four copies the selection keeps the first three; the arg-max of a row with its maximum twice is the
    lower column"""
    V, ld = 1003, 1008
    x = np.repeat(CR.make_logits(1, V, seed=3, sigma=0.25), 6, 0)
    x[:, 500] = 2.0
    x[:, 40] = 2.0                                                       # the maximum twice: columns 40 and 500
    labels = np.array([40, -1, 40, 40, 500, 40], dtype=np.int64)
    x[4] = x[4] * 0.5                                                    # a different (lower-loss or higher-loss) row among the copies
    ref = CR.captioning_loss(x, labels, 0.0, 0.25)                       # 5 labelled, k = 3
    buf, out, row_loss, correct, kept = _run(x, labels, ld, 0.0, 3, True)
    assert ref["k"] == 3 and torch.equal(kept.bool(), ref["kept"])
    assert row_loss[0] == row_loss[2] == row_loss[3] == row_loss[5]
    assert kept.tolist()[5] == 0                                         # the last of the equal rows is the one that goes
    assert correct.tolist() == [1, 0, 1, 1, 0, 1]                        # label 500 is not the arg-max: column 40 comes first


@pytest.mark.parametrize("shape", ["bert", "ragged"])
def test_plain_case_agrees_with_the_cross_entropy_kernel(shape):
    """eps = 0, no drop: the loss of lav_cross_entropy_fwd_bwd on a copy of the buffer within the fp32 bound, its gradient within one bf16 ulp"""
    from lavender_amd import hip as K
    V, ld, sigma = SHAPES[shape]
    rows, n_lab = 150, 22
    x, labels = CR.make_case(rows, V, n_lab, seed=5, sigma=sigma)
    ref = CR.captioning_loss(x, labels, 0.0, 0.0)
    b = CR.bounds(x, labels, 0.0, ld, ref)
    buf, out, *_ = _run(x, labels, ld, 0.0, n_lab, False)
    buf_ce, view_ce = _device_buffer(x, ld)
    acc = torch.zeros(2, dtype=torch.float32, device="cuda")
    K.cross_entropy(view_ce, V, torch.from_numpy(labels).cuda(), acc, 1.0 / n_lab, True)
    torch.cuda.synchronize()
    acc = acc.cpu()
    assert acc[1].item() == n_lab
    assert _ratio("caption loss - cross entropy (sum)", abs(out[0].item() - acc[0].item()), 2 * b["total"])
    g, g_ce = buf.float().cpu(), buf_ce.float().cpu()
    ulp = torch.maximum(g.abs(), g_ce.abs()) * 2.0 ** -7                 # bf16: 8 significant bits, one ulp <= 2^-7 |g|
    d = (g - g_ce).abs()
    print(f"    gradient vs cross entropy: max |d| {d.max().item():.3e}, elements that differ {int((d > 0).sum())}")
    assert (d <= ulp).all()


def test_loss_object_and_autograd_surface():
    """CaptioningLoss on a logits view: iter / drop_worst_after, the stats tensor, the upstream gradient applied on the device, keep_logits"""
    from lavender_amd.captioning import CaptioningLoss
    V, ld = 1003, 1008
    x, labels = CR.make_case(150, V, 22, seed=9, sigma=0.25)
    lab = torch.from_numpy(labels).cuda()
    lf = CaptioningLoss({"label_smoothing": 0.1, "drop_worst_ratio": 0.25, "drop_worst_after": 1})
    for call in range(2):
        buf, view = _device_buffer(x, ld)
        view.requires_grad_(True)
        ls = lf(view, lab, 22)
        ref = CR.captioning_loss(x, labels, 0.1, 0.25, drop=call + 1 > 1)
        b = CR.bounds(x, labels, 0.1, ld, ref)
        assert lf.iter == call + 1
        assert _ratio(f"call {call}: loss", abs(ls.item() - ref["loss"]), b["loss"])
        assert lf.stats.tolist()[1:] == [ref["k"], int(ref["correct"].sum()), 22]
        (0.5 * ls).backward()                                            # an upstream gradient other than 1
        torch.cuda.synchronize()
        g = view.grad.float().cpu().double()
        assert ((g - 0.5 * ref["grad"]).abs() <= 0.5 * b["grad"] + 2.0 ** -8 * (0.5 * ref["grad"]).abs()).all()
    # without the host's count: one read-back, same result; keep_logits leaves the caller's tensor alone
    lf2 = CaptioningLoss({"label_smoothing": 0.1}, keep_logits=True)
    buf, view = _device_buffer(x, ld)
    view.requires_grad_(True)
    ls = lf2(view, lab)
    ls.backward()
    torch.cuda.synchronize()
    assert torch.equal(buf[:, :V].float().cpu(), torch.from_numpy(x))
    ref = CR.captioning_loss(x, labels, 0.1, 0.0)
    assert abs(ls.item() - ref["loss"]) <= CR.bounds(x, labels, 0.1, ld, ref)["loss"]
    with torch.no_grad():                                                # evaluation: nothing is written
        buf, view = _device_buffer(x, ld)
        ls = lf2(view, lab, 22)
        assert torch.equal(buf[:, :V].float().cpu(), torch.from_numpy(x))
    with pytest.raises(ValueError, match="mean of no rows"):
        CaptioningLoss({"drop_worst_ratio": 0.25})(view, lab, 1)
