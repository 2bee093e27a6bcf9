"""Gradient clipping + Adam + weight repack (FusedPolicy.optimizer_step,
ppo_minibatch, ppo_update; bb_policy_adam_step / bb_policy_ppo_step) against
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on a float64 copy of the agent.

Bound, per tensor: max |new - f64| <= max(4 x max |torch f32 - f64|, 2^-20
|ref|_inf), the yardstick being the same torch code in float32 (the project's
bound for a different order of f32 roundings of the same formula; a misplaced
eps or bias correction, a stale packed weight or a skipped element is 10^2-10^6
times larger).  The fused path must equal ppo_grad + optimizer_step bit for bit.
"""
import copy
import ctypes

import pytest
import torch

from madrona_basketball_amd import _lib
from madrona_basketball_amd.policy import PARAMS, AdamState, FusedPolicy, make_agent
from tests.test_ppo_grad import BATCH, BIG, CLIP, ENT, VF, R, base, torch_loss

MODES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
# offset of agent.parameters()[i] in the state's packed order (bb_policy_grad.h PG_*)
OFF = [0, 4096, 4128, 4160, 4192, 5216, 5248, 5280, 5312, 5952, 5920, 5971]
W2, CRITIC = 4, (10, 11)
GRADS = {"clip": lambda g, k, i, n: torch.randn(n, generator=g) * (30 / PARAMS ** 0.5),
         "noclip": lambda g, k, i, n: torch.randn(n, generator=g) * (0.3 / PARAMS ** 0.5),
         "tiny": lambda g, k, i, n: (torch.randn(n, generator=g).sign() * 10 ** (-9 + 2 * torch.rand(n, generator=g))
                                     if i == W2 else torch.randn(n, generator=g) * 1e-2),
         "zeros": lambda g, k, i, n: torch.randn(n, generator=g) * (0.0 if k > 0 and i in (W2,) + CRITIC else 1e-2)}


def close(what, new, ref, t32):
    ref = ref.detach().double().reshape(-1)
    dev = (new.detach().double().cpu().reshape(-1) - ref).abs().max().item()
    own = (t32.detach().double().reshape(-1) - ref).abs().max().item()
    bound = max(4 * own, 2.0 ** -20 * ref.abs().max().item())
    print(f"{what}: dev {dev:.3e} torch-f32 {own:.3e} ratio {dev / max(own, 1e-300):.2f}")
    assert dev <= bound, (what, dev, own, bound)


class Ref:
    """The float64 reference and its float32 yardstick: an agent copy under
    clip_grad_norm_ + torch.optim.Adam."""

    def __init__(self, agent, dtype):
        self.agent = copy.deepcopy(agent).cpu().to(dtype)
        self.ps = list(self.agent.parameters())
        self.opt = torch.optim.Adam(self.ps, lr=3e-4, eps=1e-8)

    def step(self):
        norm = torch.nn.utils.clip_grad_norm_(self.ps, 1.0)
        self.opt.step()
        return torch.stack([norm, torch.clamp(1.0 / (norm + 1e-6), max=1.0)])

    def state(self, key):
        return [self.opt.state[p][key] for p in self.ps]


def check_state(tag, agent, state, f64, f32, grads=True):
    for i, (p, r, y) in enumerate(zip(agent.parameters(), f64.ps, f32.ps)):
        close(f"{tag} param {i}", p, r, y)
        if grads:
            close(f"{tag} grad {i}", p.grad, r.grad, y.grad)
        for key in ("exp_avg", "exp_avg_sq"):
            close(f"{tag} {key} {i}", getattr(state, key)[OFF[i]:OFF[i] + p.numel()], f64.state(key)[i], f32.state(key)[i])


@pytest.mark.parametrize("case", list(GRADS))
@pytest.mark.parametrize("mode", MODES)
def test_optimizer_step_vs_float64(native_lib, mode, case):
    agent = make_agent(3).to(mode)
    pol, state = FusedPolicy.from_agent(agent), AdamState(mode)
    f64, f32 = Ref(agent, torch.float64), Ref(agent, torch.float32)
    g = torch.Generator().manual_seed(5)
    for k in range(3):
        for i, (p, r, y) in enumerate(zip(agent.parameters(), f64.ps, f32.ps)):
            y.grad = GRADS[case](g, k, i, p.numel()).reshape(p.shape)
            r.grad, p.grad = y.grad.double(), y.grad.clone().to(mode)
        out2, r2, y2 = pol.optimizer_step(state), f64.step(), f32.step()
        if case == "noclip":
            assert out2[1].item() == 1.0
        close(f"{mode} {case} {k} out2", out2, r2, y2)
        check_state(f"{mode} {case} {k}", agent, state, f64, f32)
        assert state.step.item() == k + 1 and state.ticket.item() == 0


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("idx", [torch.arange(17) * 5, torch.randperm(R, generator=torch.Generator().manual_seed(2)),
                                 torch.arange(BIG) % R], ids=["m17", "perm", "big"])
@pytest.mark.parametrize("mode", MODES)
def test_fused_minibatch_equals_grad_then_step(native_lib, mode, idx):
    agent, _, d = base()
    agents = [copy.deepcopy(agent).to(mode) for _ in range(2)]
    pols, states = [FusedPolicy.from_agent(a) for a in agents], [AdamState(mode), AdamState(mode)]
    args = [d[k].to(mode) for k in BATCH] + [idx.to(mode)]
    for k in range(2 if mode == "cpu" else 4):  # each minibatch differentiates at the one before's packed weights
        with _lib.diag(ppo_step_ticket=k // 2):  # on the device: both forms of the fused path, twice each
            fused = pols[0].ppo_minibatch(*args, states[0], clip_coef=CLIP, vf_coef=VF, ent_coef=ENT)
        loss4 = pols[1].ppo_grad(*args, clip_coef=CLIP, vf_coef=VF, ent_coef=ENT)
        assert same_bits([fused], [torch.cat([loss4, pols[1].optimizer_step(states[1])])])
        for pa, pb in zip(agents[0].parameters(), agents[1].parameters()):
            assert same_bits([pa, pa.grad], [pb, pb.grad])
        assert same_bits([states[0].exp_avg, states[0].exp_avg_sq], [states[1].exp_avg, states[1].exp_avg_sq])
        assert states[0].step.item() == states[1].step.item() and states[0].ticket.item() == 0
    fresh = FusedPolicy.from_agent(agents[0])._tensors  # the in-kernel repack is refresh()
    for p in pols:
        assert same_bits([p._tensors[k] for k in fresh], fresh.values())
    assert not torch.equal(fresh["w1"].cpu(), FusedPolicy.from_agent(agent)._tensors["w1"])


@pytest.mark.parametrize("rows", [192, 194])
@pytest.mark.parametrize("mode", MODES)
def test_ppo_update_vs_float64_loop(native_lib, mode, rows):
    agent, norm, d = base()
    d = {k: v[torch.arange(rows) % R] for k, v in d.items()}
    perms = torch.stack([torch.randperm(rows, generator=torch.Generator().manual_seed(7 + e)) for e in range(2)])
    f64, f32 = Ref(agent, torch.float64), Ref(agent, torch.float32)
    res = {f64: [], f32: []}
    for ref in (f64, f32):
        for e in range(2):
            for start in range(0, rows, rows // 4):
                ref.opt.zero_grad()
                loss, pre, _, _ = torch_loss(ref.agent, norm, d, perms[e][start:start + rows // 4])
                if ref is f64:  # the precondition, from the reference alone: no ReLU within 1e-5 of its kink
                    assert min(y.detach().abs().min().item() for y in pre) > 1e-5
                loss[0].backward()
                res[ref].append(torch.cat([loss.detach(), ref.step()]))
    agent = copy.deepcopy(agent).to(mode)
    pol, state = FusedPolicy.from_agent(agent), AdamState(mode)
    out = pol.ppo_update(*[d[k].to(mode) for k in BATCH], state, update_epochs=2, num_minibatches=4,
                         perms=perms.to(mode), clip_coef=CLIP, vf_coef=VF, ent_coef=ENT)
    assert tuple(out.shape) == (8 + 2 * (rows % 4 != 0), 6) and state.step.item() == out.shape[0]
    for c, name in enumerate(("loss", "pg", "cl", "ent", "norm", "coef")):
        close(f"{mode} {rows} {name}", out[:, c], torch.stack(res[f64])[:, c], torch.stack(res[f32])[:, c])
    check_state(f"{mode} {rows}", agent, state, f64, f32, grads=False)


def test_step_bad_arguments(native_lib):
    L = native_lib
    agent = make_agent(1)
    pol, state = FusedPolicy.from_agent(agent), AdamState("cpu")
    for p in agent.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(ValueError):
        pol.optimizer_step(AdamState("meta"))
    _, _, d = base()
    with pytest.raises(ValueError):
        pol.ppo_minibatch(*[d[k] for k in BATCH], None, AdamState("meta"))
    ps = list(agent.parameters())
    params, grads = _lib.PolicyParams(*[p.data_ptr() for p in ps]), _lib.PolicyParams(*[p.grad.data_ptr() for p in ps])
    st = _lib.AdamStatePtrs(state.exp_avg.data_ptr(), state.exp_avg_sq.data_ptr(), state.step.data_ptr(),
                            state.ticket.data_ptr())
    hyper, out = _lib.AdamHyper(3e-4, 0.9, 0.999, 1e-8, 1.0), torch.zeros(6)

    def adam(params=params, st=st, hyper=hyper, out=out.data_ptr()):
        return L.bb_policy_adam_step(ctypes.byref(pol._w), _lib.EXEC_CPU, -1, ctypes.byref(params), ctypes.byref(grads),
                                     ctypes.byref(st), ctypes.byref(hyper), out, None)
    bad_ptr = _lib.PolicyParams(*[p.data_ptr() for p in ps[:-1]], ps[-1].data_ptr() + 2)
    assert adam(out=None) < 0 and adam(params=bad_ptr) < 0 and b"misaligned" in L.bb_last_error()
    assert adam(params=_lib.PolicyParams()) < 0 and adam(st=_lib.AdamStatePtrs(st.exp_avg, st.exp_avg_sq, None, None)) < 0
    assert adam(hyper=_lib.AdamHyper(0.0, 0.9, 0.999, 1e-8, 1.0)) < 0 and b"lr" in L.bb_last_error()
    assert state.step.item() == 0  # nothing ran
    # the fused entry in device mode: a short workspace is refused before anything is launched
    m, need = 64, L.bb_policy_ppo_step_workspace_bytes(64)
    assert need > L.bb_policy_ppo_grad_workspace_bytes(m) and L.bb_policy_ppo_step_workspace_bytes(0) == 0
    batch = _lib.PpoBatch(*[d[k].data_ptr() for k in BATCH], None, R, m)
    coef, ws = _lib.PpoCoef(CLIP, VF, ENT), torch.zeros(need // 4)

    def fused(nbytes=need, hyper=hyper, out=out.data_ptr(), batch=batch):
        return L.bb_policy_ppo_step(ctypes.byref(pol._w), _lib.EXEC_CUDA, 0, ctypes.byref(batch), ctypes.byref(coef),
                                    ctypes.byref(params), ctypes.byref(grads), ctypes.byref(st), ctypes.byref(hyper), out,
                                    ws.data_ptr(), nbytes, None)
    assert fused(nbytes=need - 1) < 0 and b"workspace" in L.bb_last_error()
    assert fused(out=None) < 0 and fused(hyper=_lib.AdamHyper(-1.0, 0.9, 0.999, 1e-8, 1.0)) < 0
    assert fused(batch=_lib.PpoBatch(None, *[d[k].data_ptr() for k in BATCH[1:]], None, R, m)) < 0
