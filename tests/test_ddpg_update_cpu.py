"""The DDPG update on the CPU (the torch path, fused=False): the replay ring against the reference's deque, train_ddpg against the
fixtures recorded from the reference's own train_ddpg (tests/golden/ddpg_update, tools/make_ddpg_update_golden.py) and against
float64 autograd of the restated losses, one real step, and the too-few-rows return."""
import copy

import pytest
import torch

from cygym_amd import ddpg_rollout as D
from ddpg_util import FIXTURES, N_UPDATES, TAU, batch_of, check_fixture_updates, expect64, f64, load_fixture, make_agent, recorded, targets_at
from ppo_util import U, tau


def _rows(lo, hi, W=3, A=2):
    i = torch.arange(lo, hi, dtype=torch.float32)
    return i[:, None] + torch.arange(W) / 8.0, -i[:, None] - torch.arange(A) / 8.0, i.double() + 0.1, 100.0 + i[:, None] + torch.arange(W) / 8.0, i % 3 == 0


def _check_rows(got, ids):
    s, a, r, s2, d = got
    want = _rows(0, 1000)
    ids = torch.as_tensor(ids)
    assert torch.equal(s, want[0][ids]) and torch.equal(a, want[1][ids]) and torch.equal(s2, want[3][ids])
    assert r.dtype == torch.float32 and r.shape == (len(ids), 1) and torch.equal(r[:, 0], want[2][ids].float())       # float64 rewards arrive as float32
    assert d.dtype == torch.float32 and d.shape == (len(ids), 1) and torch.equal(d[:, 0], want[4][ids].float())


def test_ring_keeps_the_last_rows_in_order():
    ring = D.ReplayRing(10, 3, 2, "cpu")
    assert len(ring) == 0
    for lo, hi, held in ((0, 4, 4), (4, 8, 8), (8, 13, 10)):
        ring.push(*_rows(lo, hi))
        assert len(ring) == held
    _check_rows(ring.sample_at(torch.arange(10)), range(3, 13))       # the deque dropped rows 0 .. 2
    _check_rows(ring.sample_at([9, 0]), [12, 3])
    ring = D.ReplayRing(10, 3, 2, "cpu")
    ring.push(*_rows(0, 13))                                          # one push longer than the ring: the last 10 survive
    assert len(ring) == 10
    _check_rows(ring.sample_at(torch.arange(10)), range(3, 13))
    ring.push(*_rows(13, 15))
    _check_rows(ring.sample_at(torch.arange(10)), range(5, 15))


def test_ring_sample_is_distinct_reproducible_and_refuses_too_many():
    ring = D.ReplayRing(10, 3, 2, "cpu")
    ring.push(*_rows(0, 13))
    draws = []
    for _ in range(2):
        s, a, r, s2, d = ring.sample(6, torch.Generator().manual_seed(5))
        ids = (r[:, 0] - 0.1).round().long()
        assert len(set(ids.tolist())) == 6 and all(3 <= i < 13 for i in ids.tolist())
        _check_rows((s, a, r, s2, d), ids)
        draws.append(ids)
    assert torch.equal(draws[0], draws[1])
    assert not torch.equal(draws[0], (ring.sample(6, torch.Generator().manual_seed(6))[2][:, 0] - 0.1).round().long())
    with pytest.raises(ValueError, match="fewer"):
        ring.sample(11)
    seen = set()
    g = torch.Generator().manual_seed(0)
    for _ in range(40):
        seen |= set((ring.sample(3, g)[2][:, 0] - 0.1).round().long().tolist())
    assert seen == set(range(3, 13))                                  # every row held can be drawn


def test_ring_takes_transitions_in_t_n_order():
    T, N = 3, 2
    s, a, r, s2, d = _rows(0, T * N)
    tr = D.Transitions(state=s.reshape(T, N, 3), action_vec=a.reshape(T, N, 2), reward=r.reshape(T, N), raw_reward=r.reshape(T, N),
                       next_state=s2.reshape(T, N, 3), done=d.reshape(T, N), noise_std=0.0)
    ring = D.ReplayRing(10, 3, 2, "cpu")
    ring.push(tr)
    assert len(ring) == 6
    _check_rows(ring.sample_at(torch.arange(6)), range(6))


@pytest.mark.parametrize("name", FIXTURES)
def test_recorded_batches_walk_the_clamp_and_both_smooth_l1_branches(name):
    z, sd, tsd = load_fixture(name)
    for i in range(N_UPDATES):
        s, a, r, s2, d = batch_of(z, i)
        want = expect64(f64(sd["actor"]), f64(sd["critic"]), targets_at(sd, tsd, i), (s, a, r, s2, d), float(z["gamma"]))
        delta = (want["q"] - want["td"]).abs()
        assert bool((r.abs() > 10).any()) and bool(d.any()) and bool((delta < 1).any()) and bool((delta > 1).any()), (name, i, r, delta)


@pytest.mark.parametrize("name", FIXTURES)
def test_train_ddpg_on_the_recorded_updates(name):
    check_fixture_updates(name, fused=False)


def test_one_real_step():
    """def12 nets, SGD lr 0.05 on both: the parameters after train_ddpg against p - lr scale g64 with scale = min(1, 0.5 / (n64 + 1e-6)),
    within lr tau(g) + 2 u max |want|.  The actor's gradient is taken through the UPDATED critic: the expectation built that way
    holds, the one built from the old critic misses by more than the bound."""
    lr = 0.05
    z, sd, tsd = load_fixture("def12")
    gamma = float(z["gamma"])
    agent = make_agent(z, sd, tsd, lr)
    sample = batch_of(z, 0)
    tgt0 = {"critic": copy.deepcopy(agent.target_critic.state_dict()), "actor": copy.deepcopy(agent.target_actor.state_dict())}
    out = D.train_ddpg(agent, fused=False, sample=sample, gamma=gamma)
    old = expect64(f64(sd["actor"]), f64(sd["critic"]), targets_at(sd, tsd, 0), sample, gamma)
    scale = lambda n: min(1.0, 0.5 / (n + 1e-6))  # noqa: E731
    want_c = {k: sd["critic"][k].double() - lr * scale(old["n_critic"]) * g for k, g in old["g_critic"].items()}
    new = expect64(f64(sd["actor"]), f64(sd["critic"]), targets_at(sd, tsd, 0), sample, gamma, critic_for_actor=want_c)
    rec_c, rec_a = recorded(z, "critic", "g0"), recorded(z, "actor", "g0")

    def miss(model, start, g64, n64, e_ref_of):
        worst = 0.0
        for k, p in model.named_parameters():
            want = start[k].double() - lr * scale(n64) * g64[k]
            bound = lr * tau(g64[k], g64[k] + e_ref_of(k)) + 2.0 * U * float(want.abs().max())
            worst = max(worst, float((p.detach().double() - want).abs().max()) / bound)
        return worst

    # e_ref: the recorded gradient's own distance from float64 (taken at the old critic for the actor: the same arithmetic, the same size);
    # a tensor the fixture holds no gradient of gets the floor 8 u max |g64| of tau alone
    e_c = lambda k: (rec_c[k].double() - old["g_critic"][k]) if k in rec_c else torch.zeros(())  # noqa: E731
    e_a = lambda k: (rec_a[k].double() - old["g_actor"][k]) if k in rec_a else torch.zeros(())  # noqa: E731
    m_c = miss(agent.critic, sd["critic"], old["g_critic"], old["n_critic"], e_c)
    m_new = miss(agent.actor, sd["actor"], new["g_actor"], new["n_actor"], e_a)
    m_old = miss(agent.actor, sd["actor"], old["g_actor"], old["n_actor"], e_a)
    print(f"largest |p - want| / bound: critic {m_c:.3g}, actor through the updated critic {m_new:.3g}, through the old critic {m_old:.3g}")
    assert m_c <= 1.0 and m_new <= 1.0 and m_old > 1.0, (m_c, m_new, m_old)
    assert abs(float(out["critic_grad_norm"]) - old["n_critic"]) <= 1e-5 * old["n_critic"] and abs(float(out["actor_grad_norm"]) - new["n_actor"]) <= 1e-5 * new["n_actor"]
    # the targets: tau src + (1 - tau) tgt on the UPDATED nets, the reference's expression in fp32
    for net, model, src in (("critic", agent.target_critic, agent.critic), ("actor", agent.target_actor, agent.actor)):
        for (k, t), p in zip(model.named_parameters(), src.parameters()):
            assert torch.equal(t.detach(), TAU * p.detach() + (1 - TAU) * tgt0[net][k]), (net, k)
    # after the call critic.*.grad holds the critic loss's gradients (clipped), not the actor loss's
    c = scale(old["n_critic"])
    for k, p in agent.critic.named_parameters():
        assert float((p.grad.double() - c * old["g_critic"][k]).abs().max()) <= c * tau(old["g_critic"][k], old["g_critic"][k] + e_c(k)) + 2.0 * U * float(old["g_critic"][k].abs().max())


def test_too_few_rows_returns_none_and_changes_nothing():
    z, sd, tsd = load_fixture("def12")
    agent = make_agent(z, sd, tsd, 0.05)
    s, a, r, s2, d = batch_of(z, 0)
    agent.replay.push(s[:11], a[:11], r[:11], s2[:11], d[:11])
    before = [p.detach().clone() for net in (agent.actor, agent.critic, agent.target_actor, agent.target_critic) for p in net.parameters()]
    assert D.train_ddpg(agent, batch_size=12, fused=False) is None
    after = [p for net in (agent.actor, agent.critic, agent.target_actor, agent.target_critic) for p in net.parameters()]
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    agent.replay.push(s[11:], a[11:], r[11:], s2[11:], d[11:])          # the twelfth row: now it trains, from the ring
    out = D.train_ddpg(agent, batch_size=12, fused=False, generator=torch.Generator().manual_seed(1))
    assert set(out) == {"critic_loss", "actor_loss", "critic_grad_norm", "actor_grad_norm"} and all(v.dim() == 0 and bool(torch.isfinite(v)) for v in out.values())
    assert not torch.equal(before[0], next(agent.actor.parameters()))
