"""GPU: the classifier two-sample test on the device (cd_classifier_*, cd_op_linear_act*, calodiffusion_amd.classifier) against the
restatement of classifier_cases.py.  The layer kernels are checked bit for bit on integers; logits, gradients, losses and trained
parameters against the float64 restatement at 4 x the error of its own fp32 torch-CPU evaluation (each figure is printed).

Worst device error / fp32-CPU error seen on an MI355X (relative L2 per tensor; the bound is 4): see DESIGN.md section 8h."""
import math

import numpy as np
import pytest
import torch

import classifier_cases as K
from calodiffusion_amd import classifier as CL

pytestmark = pytest.mark.gpu

P = 0.2


def cuda(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def device_model(model):
    """(desc, [fp32 device parameter tensors in parameters() order]) of a restated module."""
    d, h = model.inputlayer.in_features, model.inputlayer.out_features
    num_layer = sum(isinstance(l, torch.nn.Linear) for l in model.layers) - 2
    return CL._desc(d, h, num_layer, K.SLOPE, model.dpo), [p.detach().float().cuda().contiguous() for p in model.parameters()]


def device_masks(seed, step, layers, p, rows, hidden):
    return [CL.dropout_mask(seed, step, l, p, rows, hidden).cpu() for l in range(layers)]


def show(report):
    for name, e_dev, e_32, ratio in report:
        print(f"    {name:28s} device {e_dev:.3e}  fp32-cpu {e_32:.3e}  ratio {ratio:.2f}")


# ---- 1. layout on integers, bitwise ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("first_layer", [True, False])
def test_layer_kernels_on_integers(shape, first_layer):
    """cd_op_linear_act / cd_op_linear_act_backward, exact: a misplaced fragment element, a padded column that leaks or a mask
    indexed by anything but (row-in-batch, column) is an O(1) error."""
    d, hidden, _, batch = shape
    n_in = d if first_layer else hidden
    case = K.integer_layer_case(batch, n_in, hidden, seed=17 * d + hidden + batch)
    seed, step, layer = 99, 7, 2
    mask = CL.dropout_mask(seed, step, layer, K.INT_P, batch, hidden)
    want = K.integer_layer_reference(case, mask.cpu().numpy())
    x, w, b, dy = (cuda(case[k]) for k in ("x", "w", "b", "dy"))
    y = CL.linear_act(x, w, b, True, K.INT_SLOPE, K.INT_P, seed, step, layer)
    assert K.same_bits(y.cpu().numpy(), want["y"])
    dx, dw, db = CL.linear_act_backward(x, w, y, dy, mask, K.INT_SCALE, True, K.INT_SLOPE)
    for name, got in (("dx", dx), ("dw", dw), ("db", db)):
        assert K.same_bits(got.cpu().numpy(), want[name]), name
    # without a mask and without an activation: the plain products
    y0 = CL.linear_act(x, w, None, False)
    assert K.same_bits(y0.cpu().numpy(), case["x"].astype(np.float64) @ case["w"].astype(np.float64).T)
    dx0, dw0, db0 = CL.linear_act_backward(x, w, y0, dy, None, 1.0, False)
    dy64 = case["dy"].astype(np.float64)
    assert K.same_bits(dx0.cpu().numpy(), dy64 @ case["w"]) and K.same_bits(dw0.cpu().numpy(), dy64.T @ case["x"])
    assert K.same_bits(db0.cpu().numpy(), dy64.sum(axis=0))


# ---- 2. forward ------------------------------------------------------------------------------------------------------------------------

NETS = sorted({s[:3] for s in K.SHAPES})


@pytest.mark.parametrize("net", NETS)
def test_forward_logits(net):
    d, hidden, num_layer = net
    m64 = K.make_model(d, hidden, num_layer, 0.0, seed=d)
    m32 = K.clone_as(m64, torch.float32)
    desc, params = device_model(m64)
    x, _ = K.seeded_rows(1000, d, seed=hidden)
    rng = np.random.default_rng(d)
    xd, report, ok = cuda(x), [], True
    with torch.no_grad():
        for rows in (1, 255, 257, 1000):
            idx = rng.integers(0, 1000, size=rows)
            idx[: rows // 3] = idx[0]  # repeats
            for tag, sel in (("first rows", np.arange(rows)), ("index list", idx)):
                want = m64(torch.from_numpy(x[sel]).double()).reshape(-1).numpy()
                ref32 = m32(torch.from_numpy(x[sel])).reshape(-1).numpy()
                if tag == "first rows":
                    got = CL.forward_logits(desc, params, xd, count=rows, max_rows_per_call=256)
                else:
                    got = CL.forward_logits(desc, params, xd, idx=cuda(sel, torch.int32), max_rows_per_call=256)
                ok &= K.within_four_times(f"{rows} rows, {tag}", got.cpu().numpy(), ref32, want, report)
    show(report)
    assert ok, report


def test_dnn_module_forward_and_bad_index():
    m = CL.DNN(1, 40, 33).cuda().eval()
    ref = K.RestatedDNN(1, 40, 33)
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    x, _ = K.seeded_rows(70, 33, seed=1)
    got = m(cuda(x))
    assert got.shape == (70, 1) and K.rel_l2(got.cpu().numpy(), ref.double()(torch.from_numpy(x).double()).detach().numpy()) < 1e-5
    m.train()
    with pytest.raises(NotImplementedError, match="ClassifierTest.fit"):
        m(cuda(x))
    with torch.no_grad():
        assert torch.equal(m(cuda(x)), got)  # train mode under no_grad scores without dropout
    # an index outside the matrix is never dereferenced: its logit is NaN, the others are untouched
    idx = cuda(np.array([0, 70, 3, -1, 69]), torch.int32)
    z = CL.forward_logits(m.desc(), m.device_params(), cuda(x), idx=idx).cpu().numpy()
    assert np.isnan(z[[1, 3]]).all() and np.array_equal(z[[0, 2, 4]], got.cpu().numpy().reshape(-1)[[0, 3, 69]])


# ---- 3. one training step, then twenty ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", K.SHAPES)
def test_training_step_gradients(shape):
    d, hidden, num_layer, batch = shape
    m64 = K.make_model(d, hidden, num_layer, P, seed=hidden + batch)
    m32 = K.clone_as(m64, torch.float32)
    desc, params = device_model(m64)
    x, y = K.seeded_rows(300, d, seed=batch)
    idx = np.random.default_rng(3).permutation(300)[:batch]
    seed, step = 11, 5
    masks = device_masks(seed, step, num_layer + 1, P, batch, hidden)
    loss64, g64 = K.loss_and_grads(m64, x[idx], y[idx], masks)
    loss32, g32 = K.loss_and_grads(m32, x[idx], y[idx], masks)
    grads = torch.full((CL.num_params(desc),), 7.0, device="cuda")  # a sentinel: every element is written
    before = [p.clone() for p in params]
    loss = CL.train_step(desc, params, cuda(x), cuda(y), cuda(idx, torch.int32), seed, step, grads)
    assert all(torch.equal(a, b) for a, b in zip(before, params))  # no Adam asked for: the weights stay
    got, at, report, ok = grads.cpu().numpy(), 0, [], True
    names = [n for n, _ in m64.named_parameters()]
    for name, a, b in zip(names, g64, g32):
        n = a.numel()
        ok &= K.within_four_times(name, got[at:at + n], b.numpy(), a.numpy(), report)
        at += n
    assert at == got.size
    ok &= K.within_four_times("loss", [loss.item()], [loss32], [loss64], report)
    show(report)
    assert ok, report


@pytest.mark.parametrize("shape,rows", [((5, 72, 2, 37), 20 * 37 - 9), ((226, 2024, 2, 256), 20 * 256)])
def test_twenty_adam_steps(shape, rows):
    """One cd_classifier_train_epoch call of 20 steps (the last batch ragged at the small shape) against torch.optim.Adam on the
    restatement with the device's masks: parameters after the last step, and the per-step losses."""
    d, hidden, num_layer, batch = shape
    lr, seed = 1e-4, 5
    m64 = K.make_model(d, hidden, num_layer, P, seed=rows)
    m32 = K.clone_as(m64, torch.float32)
    desc, params = device_model(m64)
    x, y = K.seeded_rows(rows + 50, d, seed=d)
    perm = np.random.default_rng(8).permutation(rows + 50)[:rows]
    batches = [perm[lo:lo + batch] for lo in range(0, rows, batch)]
    assert len(batches) == 20
    masks = [device_masks(seed, k, num_layer + 1, P, len(b), hidden) for k, b in enumerate(batches)]
    n = CL.num_params(desc)
    grads, m, v = (torch.zeros((n,), device="cuda") for _ in range(3))
    losses = CL.train_epoch(desc, params, cuda(x), cuda(y), cuda(perm, torch.int32), batch, seed, 0, grads, m, v, lr)
    assert losses.shape == (20,)
    l64 = K.adam_steps(m64, x, y, batches, masks, lr)
    l32 = K.adam_steps(m32, x, y, batches, masks, lr)
    report, ok = [], True
    for (name, a), b, got in zip(m64.named_parameters(), m32.parameters(), params):
        ok &= K.within_four_times(name, got.cpu().numpy(), b.detach().numpy(), a.detach().numpy(), report)
    ok &= K.within_four_times("losses", losses.cpu().numpy(), l32, l64, report)
    show(report)
    assert ok, report


def test_epoch_equals_its_steps():
    """cd_classifier_train_epoch from first_step 0 is bitwise the chain of cd_classifier_train_step calls."""
    d, hidden, num_layer, batch, rows = 5, 72, 2, 37, 5 * 37 - 4
    m = K.make_model(d, hidden, num_layer, P, seed=2)
    desc, pa = device_model(m)
    _, pb = device_model(m)
    x, y = K.seeded_rows(rows, d, seed=4)
    xd, yd, perm = cuda(x), cuda(y), np.random.default_rng(1).permutation(rows)
    n = CL.num_params(desc)
    ga, ma, va, gb, mb, vb = (torch.zeros((n,), device="cuda") for _ in range(6))
    la = CL.train_epoch(desc, pa, xd, yd, cuda(perm, torch.int32), batch, 3, 0, ga, ma, va, 1e-3)
    lb = [CL.train_step(desc, pb, xd, yd, cuda(perm[lo:lo + batch], torch.int32), 3, k, gb, adam=(mb, vb, 1e-3, 0.9, 0.999, 1e-8, k + 1))
          for k, lo in enumerate(range(0, rows, batch))]
    assert torch.equal(la, torch.cat(lb)) and all(torch.equal(a, b) for a, b in zip(pa, pb)) and torch.equal(ga, gb)


# ---- 4. dropout mask -------------------------------------------------------------------------------------------------------------------

def test_dropout_mask():
    rows, n, layers = 256, 2024, 3
    masks = [CL.dropout_mask(21, 4, l, P, rows, n) for l in range(layers)]
    kept = sum(int(m.sum().item()) for m in masks)
    total = rows * n * layers
    sigma = math.sqrt(P * (1 - P) / total)
    assert abs(kept / total - (1 - P)) <= 6 * sigma, (kept / total, sigma)
    assert all(set(np.unique(m.cpu().numpy())) <= {0, 1} for m in masks)
    assert torch.equal(masks[1], CL.dropout_mask(21, 4, 1, P, rows, n))  # the same key, the same bytes
    assert not torch.equal(masks[1], masks[2]) and not torch.equal(masks[1], CL.dropout_mask(21, 5, 1, P, rows, n))
    assert not torch.equal(masks[1], CL.dropout_mask(22, 4, 1, P, rows, n))
    assert not torch.equal(masks[1], CL.dropout_mask(21, 4 + 2 ** 32, 1, P, rows, n))  # the high word of the step counts
    assert torch.equal(masks[0][:37], CL.dropout_mask(21, 4, 0, P, 37, n))  # a ragged batch is the head of a full one
    assert bool(CL.dropout_mask(21, 4, 0, 0.0, 5, 9).all())


def test_mask_follows_the_place_in_the_batch_not_the_row():
    """Two batches that list different matrix rows holding the same features get the same gradient: the mask of row-in-batch r does
    not depend on which matrix row sits there."""
    d, hidden, num_layer, batch = 5, 72, 2, 37
    m = K.make_model(d, hidden, num_layer, P, seed=1)
    desc, params = device_model(m)
    x, y = K.seeded_rows(batch, d, seed=9)
    x2, y2 = np.concatenate([x, x[::-1]]), np.concatenate([y, y[::-1]])  # row batch + j holds the features of row batch - 1 - j
    n = CL.num_params(desc)
    g1, g2 = torch.zeros((n,), device="cuda"), torch.zeros((n,), device="cuda")
    l1 = CL.train_step(desc, params, cuda(x2), cuda(y2), cuda(np.arange(batch), torch.int32), 1, 2, g1)
    l2 = CL.train_step(desc, params, cuda(x2), cuda(y2), cuda(2 * batch - 1 - np.arange(batch), torch.int32), 1, 2, g2)
    assert torch.equal(g1, g2) and torch.equal(l1, l2)


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(5, 72, 2, 37), (226, 2024, 2, 256)])
def test_five_steps_twice_are_bitwise_equal(shape):
    d, hidden, num_layer, batch = shape
    m = K.make_model(d, hidden, num_layer, P, seed=6)
    x, y = K.seeded_rows(5 * batch, d, seed=2)
    xd, yd, perm = cuda(x), cuda(y), cuda(np.random.default_rng(0).permutation(5 * batch), torch.int32)
    runs = []
    for _ in range(2):
        desc, params = device_model(m)
        n = CL.num_params(desc)
        g, mm, vv = (torch.zeros((n,), device="cuda") for _ in range(3))
        losses = CL.train_epoch(desc, params, xd, yd, perm, batch, 13, 0, g, mm, vv, 1e-3)
        runs.append((params, losses.clone(), g))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------

def run_test(shift, seed):
    feats, labels = K.two_gaussians(4096, 5, shift, seed=seed)
    t = CL.ClassifierTest(5, num_hidden=72, dropout=0.0, n_epochs=10, seed=seed)
    start = {k: v.clone() for k, v in t.model.state_dict().items()}
    t.fit(feats, labels)
    return t, feats, labels, start


def test_end_to_end_two_gaussians():
    t, feats, labels, start = run_test(1.0, seed=0)
    res = t.evaluate()
    ref = K.RestatedDNN(2, 72, 5, 0.0)
    ref.load_state_dict(start)
    perms = [t.epoch_permutation(e) for e in range(10)]
    z_ref, best_ref = K.restated_fit(ref.double(), CL.standard_scale(feats).astype(np.float32), labels, t.split, perms, 1e-4, 256, 10)
    y_test = labels[t.split[1]].astype(np.float64)
    auc_ref = CL.roc_auc(y_test, z_ref)
    n_pos, n_neg = int(y_test.sum()), int((1 - y_test).sum())
    se = K.hanley_mcneil_se(auc_ref, n_pos, n_neg)
    print(f"    device AUC {res.auc:.4f}, restated fp64 AUC {auc_ref:.4f}, optimum {0.5 * (1 + math.erf(0.5)):.4f}, "
          f"SE {se:.4f} for {n_pos} + {n_neg} rows; best epoch {res.best_epoch} / {best_ref}")
    assert abs(res.auc - auc_ref) <= se
    z = t.logits(t.split[1])
    assert res.bce == CL.bce_with_logits(z, y_test) and res.jsd == 1.0 - res.bce / math.log(2.0)
    assert res.step_losses.shape == (10 * math.ceil(len(t.split[0]) / 256),) and np.isfinite(res.step_losses).all()
    assert res.step_losses[-20:].mean() < res.step_losses[:20].mean()
    assert 1 <= res.best_epoch <= 10 and 0.0 <= res.auc_cal <= 1.0 and res.jsd_cal <= 1.0
    rounded = t.evaluate(rounded_scores=True)
    hard = (z > 0).astype(np.float64)
    balanced = 0.5 * (np.mean(hard[y_test == 1] == 1) + np.mean(hard[y_test == 0] == 0))
    assert abs(rounded.auc - balanced) < 1e-12 and rounded.accuracy == res.accuracy and rounded.bce == res.bce


def test_end_to_end_identical_distributions():
    t, _, labels, _ = run_test(0.0, seed=1)
    res = t.evaluate()
    y_test = labels[t.split[1]]
    se = K.hanley_mcneil_se(0.5, int(y_test.sum()), int((1 - y_test).sum()))
    print(f"    AUC {res.auc:.4f}, SE {se:.4f}")
    assert abs(res.auc - 0.5) <= 3 * se


# ---- 7. hgcal_features ---------------------------------------------------------------------------------------------------------------

def test_hgcal_features():
    rng = np.random.default_rng(12)
    N, L, C = 64, 4, 37
    showers = (rng.random((N, L, C)) ** 4 * 50).astype(np.float32)
    showers[:, 2, :] = 0.0   # an empty layer
    showers[5] = 0.0         # an empty shower
    xmap, ymap = rng.uniform(-80, 80, (L, C + 3)), rng.uniform(-150, 20, (L, C + 3))  # wider tables: only [:, :C] counts
    e_inc = rng.uniform(10, 500, (N, 1))
    got = CL.hgcal_features(showers, e_inc, xmap, ymap).astype(np.float64)
    want = K.restate_compute_feats(showers, e_inc, xmap, ymap)
    assert got.shape == want.shape == (N, 2 + 5 * L)
    u = 2.0 ** -23
    blocks = {"x centre": 2 + L, "x width": 2 + 2 * L, "y centre": 2 + 3 * L, "y width": 2 + 4 * L}
    assert np.all(np.abs(got[:, :2 + L] - want[:, :2 + L]) <= u * np.abs(want[:, :2 + L]))  # E_inc, E_tot / E_inc, log10(E_layer + 1e-8)
    for name, at in blocks.items():
        table = xmap if name[0] == "x" else ymap
        err = np.abs(got[:, at:at + L] - want[:, at:at + L])
        if "centre" in name:
            assert np.all(err <= u * np.abs(table[:, :C]).max(axis=1)), name
        else:
            assert np.all(err <= u * np.abs(want[:, at:at + L])), name
        # cd_hlf_compute divides by E + 1e-16 where the reference masks E = 0: both give 0 for an empty layer and shower
        assert np.all(got[:, at + 2] == 0.0) and np.all(want[:, at + 2] == 0.0) and np.all(got[5, at:at + L] == 0.0), name
    assert np.all(got[:, 2 + 2] == np.float32(np.log10(1e-8)))


# ---- evaluate.ClassifierScore ----------------------------------------------------------------------------------------------------------

class _StubModel:
    """What a metric object uses of a trained model: config["NSTEPS"] and generate()."""

    def __init__(self, showers, energies):
        self.config = {"NSTEPS": 7}
        self.showers, self.energies, self.calls = showers, energies, []

    def generate(self, data_loader, sample_steps, sample_offset):
        self.calls.append((sample_steps, sample_offset, data_loader))
        return self.showers, self.energies


def test_classifier_score_call():
    """Generated showers 100 x brighter than the loader's: every log10(E_layer) column is shifted by 2, several times its spread (a
    layer's energy is led by its few brightest voxels, drawn over six decades), so the two sets are separable and a trained
    classifier's AUC is near 1; 0.9 leaves room for the empty shower of each set and for 80 Adam steps.  The score is
    ClassifierTest's AUC on the labelled feature arrays (generated 1, Geant4 0), bit for bit."""
    import hlf_cases as H
    from calodiffusion_amd import evaluate as E
    geo = H.Geometry.of_fixture("small")
    V, n = geo.edges[-1], 600
    rng = np.random.default_rng(41)
    ref_showers, gen_showers = H.seeded_showers(V, n, 42), H.seeded_showers(V, n, 43) * np.float32(100.0)
    ref_energy, gen_energy = rng.uniform(1e3, 1e6, (n, 1)), rng.uniform(1e3, 1e6, (n, 1))
    loader = [(torch.from_numpy(ref_energy[lo:lo + 200]), None, torch.from_numpy(ref_showers[lo:lo + 200])) for lo in range(0, n, 200)]
    model = _StubModel(gen_showers, gen_energy)
    kw = dict(num_hidden=72, dropout=0.2, n_epochs=20, lr=1e-3, seed=3)
    score = E.ClassifierScore(H.binning("small"), "electron", **kw)
    value = score(model, loader, {})
    assert model.calls == [(7, 0, loader)]
    gen, real = score.feature_arrays(_StubModel(gen_showers, gen_energy), loader)
    t = CL.ClassifierTest(gen.shape[1], **kw).fit(np.concatenate([gen, real]), np.concatenate([np.ones(n), np.zeros(n)]))
    print(f"    ClassifierScore = {value:.4f}, best epoch {score.last_result.best_epoch}, JSD {score.last_result.jsd:.4f}")
    assert isinstance(value, float) and value == score.last_result.auc == t.evaluate().auc  # a run is reproducible bit for bit
    assert value > 0.9
    score.hlf.close()
    score.reference_hlf.close()
