"""Batched learned-model controllers on the GPU (mppi_create_batch_learned, mppi_batch_set_mlp; k_rollout_nn_batch): B controllers of
NNAUVModel / NNAUVModelSpeed, each member with its OWN network, stepped in the same two launches as one.

The contract (include/mppi_c.h): member m is BIT FOR BIT the lone Handle of its config and network running k_rollout_gen<MODEL, HID, DIAG>
— the default for NNAUVModel Dense(16), else tuned with mlp32_valu = 1 — fed the same x, goal and sequence on the same step counter.
Against the oracle a member is held to the bars of the lone learned handles (tests/test_auv_gpu.py). The case matrix and its conditioning:
batch_nn_util.py, test_batch_nn_oracle.py."""
import ctypes as C

import numpy as np
import pytest

import batch_nn_util as N
from batch_util import raw_configs, rexrov2

pytestmark = pytest.mark.gpu
F32 = np.float32
CASE_IDS = range(len(N.CASES))


@pytest.fixture(scope="module")
def m():
    import __graft_entry__ as g
    g.build()
    import mppi_tf_amd as mod
    return mod


def assert_member_equals_lone(m, hb, i, h, ub, ul, tag):
    msg = "member %d %s" % (i, tag)
    for what in (m.DBG_COSTS, m.DBG_BETA, m.DBG_ETA, m.DBG_U_UPDATED):
        np.testing.assert_array_equal(hb.debug_get(i, what), h.debug_get(what), err_msg=msg)
    np.testing.assert_array_equal(ub[i], ul, err_msg=msg)


# ---- 1. member = lone handle, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", CASE_IDS, ids=N.IDS)
def test_member_equals_its_lone_handle_bit_for_bit(m, ci):
    """three consecutive steps (the warm start shifts, the Philox counter advances): costs, beta, eta, U' and u of every checked member"""
    case, mem = N.CASES[ci], N.members(ci)
    hb = N.make_batch(m, case, mem)
    assert hb.rollout_kernel_name() == N.kernel_names(case)[0]
    lone = {i: N.make_lone(m, case, mem, i) for i in N.checked(case)}
    X = mem["X"].copy()
    for step in range(3):
        ub = hb.next(X)
        assert np.isfinite(ub).all()
        for i, h in lone.items():
            assert_member_equals_lone(m, hb, i, h, ub, h.next(X[i]), "step %d" % step)
        X[:, :3] += F32(0.01)  # a new x every step
    Ub = hb.get_action_sequences()
    for i, h in lone.items():
        np.testing.assert_array_equal(Ub[i], h.get_action_sequence())
        h.close()
    assert hb.get_step_counter() == 3
    hb.close()


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", CASE_IDS, ids=N.IDS)
def test_member_against_the_oracle(m, ci):
    """the member's own noise (debug_get) through the oracle in fp32 and fp64: the bars of the lone learned handles"""
    case, mem = N.CASES[ci], N.members(ci)
    hb = N.make_batch(m, case, mem)
    hb.next(mem["X"])
    Ub = hb.get_action_sequences()  # (the shifted U', as the oracle returns it)
    for i in N.checked(case):
        noise = hb.debug_get(i, m.DBG_NOISE)
        np.testing.assert_allclose(noise, N.first_noise(case, mem, i), rtol=0, atol=5e-6)
        ref = N.oracle_step(case, mem, i, mem["U0"][i], noise)
        c = hb.debug_get(i, m.DBG_COSTS).astype(np.float64)
        rel = float((np.abs(c - ref["c64"]) / np.abs(ref["c64"])).max())
        eu = float(np.abs(Ub[i].astype(np.float64) - ref["U64"]).max())
        print("%s member %d: rel cost err GPU %.3g / CPU %.3g; max|dU'| GPU %.3g / CPU %.3g" % (case["id"], i, rel, ref["rel32"], eu, ref["eu32"]))
        assert rel < N.COST_BAR and rel < N.COST_FAC * max(ref["rel32"], 1e-6), "member %d" % i
        assert eu <= ref["u_bar"], "member %d" % i
    hb.close()


# ---- 3. independence --------------------------------------------------------------------------------------------------------------------
def test_set_mlp_moves_one_member_and_no_other(m):
    from mppi_tf_amd import _lib as L
    ci = 0
    case, mem = N.CASES[ci], N.members(ci)
    other = N.make_net(case, 999)
    a, b = N.make_batch(m, case, mem), N.make_batch(m, case, mem)
    b.set_mlp(1, other)
    ua, ub = a.next(mem["X"]), b.next(mem["X"])
    eps = N.first_noise(case, mem, 1)
    bar = N.oracle_step(case, mem, 1, mem["U0"][1], eps)["u_bar"]
    assert np.abs(ua[1] - ub[1]).max() > 100 * bar
    for i in (0, 2):
        np.testing.assert_array_equal(ua[i], ub[i])
        np.testing.assert_array_equal(a.debug_get(i, m.DBG_COSTS), b.debug_get(i, m.DBG_COSTS))
        np.testing.assert_array_equal(a.debug_get(i, m.DBG_U_UPDATED), b.debug_get(i, m.DBG_U_UPDATED))
    h = N.make_lone(m, case, mem, 1, net=other)  # ... and member 1 is the lone handle of the new network
    np.testing.assert_array_equal(ub[1], h.next(mem["X"][1]))
    np.testing.assert_array_equal(b.debug_get(1, m.DBG_COSTS), h.debug_get(m.DBG_COSTS))
    # other widths: refused, and nothing changes
    wrong = N.make_net(dict(case, hid=16), 5)
    with pytest.raises(m.MppiError) as e:
        b.set_mlp(0, wrong)
    assert e.value.status == L.ERR_INVALID_ARG and "widths" in str(e.value)
    for bad in (3, -2):
        with pytest.raises(m.MppiError) as e:
            b.set_mlp(bad, other)
        assert e.value.status == L.ERR_INVALID_ARG and "member" in str(e.value)
    a.set_mlp(1, other)  # now a holds b's networks: from the same sequences (the step counters are equal) the two agree in every member
    a.set_action_sequences(mem["U0"])
    b.set_action_sequences(mem["U0"])
    np.testing.assert_array_equal(a.next(mem["X"]), b.next(mem["X"]))
    h.close(), a.close(), b.close()


def test_set_mlp_of_every_member_makes_equal_members_equal(m):
    ci = 0
    case, mem = N.CASES[ci], N.members(ci)
    same = dict(mem, seeds=[7] * 3, lams=[1.0] * 3, G=np.tile(mem["G"][0], (3, 1)), U0=np.tile(mem["U0"][0], (3, 1, 1)))
    hb = N.make_batch(m, case, same)
    X = np.tile(mem["X"][0], (3, 1))
    u = hb.next(X)
    assert np.abs(u[0] - u[1]).max() > 0 and np.abs(u[0] - u[2]).max() > 0  # their networks differ
    hb.set_mlp(-1, mem["nets"][2])
    hb.set_action_sequences(same["U0"])
    u = hb.next(X)
    np.testing.assert_array_equal(u[0], u[1])
    np.testing.assert_array_equal(u[0], u[2])
    np.testing.assert_array_equal(hb.debug_get(0, m.DBG_COSTS), hb.debug_get(2, m.DBG_COSTS))
    hb.close()


# ---- 4. the device path -------------------------------------------------------------------------------------------------------------------
def test_next_device_on_a_torch_stream_equals_next(m):
    import torch
    ci = 3
    case, mem = N.CASES[ci], N.members(ci)
    a, b = N.make_batch(m, case, mem), N.make_batch(m, case, mem)
    st = torch.cuda.Stream()
    xd, ud = torch.tensor(mem["X"], device="cuda"), torch.zeros(case["B"], 6, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        b.next_device(xd.data_ptr(), ud.data_ptr(), st)
        st.synchronize()
        np.testing.assert_array_equal(ud.cpu().numpy(), a.next(mem["X"]))
    a.close(), b.close()


# ---- 5. episodes ----------------------------------------------------------------------------------------------------------------------
EP = dict(id="episode", model="nnauv", hid=32, nh=2, dense=False, cost="quadratic", K=128, H=6, B=3)
EP_STEPS = 4


def _episode_members():
    rng = np.random.default_rng(77)
    B, H = EP["B"], EP["H"]
    G = np.tile(N.GOAL13, (B, 1))
    G[:, :3] += rng.uniform(-1, 1, (B, 3))
    X = np.tile(N.X0, (B, 1))
    X[:, :3] += rng.uniform(-0.5, 0.5, (B, 3))
    mem = dict(nets=[N.make_net(EP, 300 + i) for i in range(B)], seeds=[5, 9, 13], lams=[0.9, 1.0, 1.2], G=G.astype(F32), X=X.astype(F32),
               U0=(0.1 * rng.standard_normal((B, H, 6))).astype(F32))
    goals = np.tile(G[None], (EP_STEPS, 1, 1)).astype(F32)
    goals[:, :, :3] += rng.uniform(-0.2, 0.2, (EP_STEPS, B, 3)).astype(F32)
    W = np.zeros((EP_STEPS, B, 13), F32)
    W[:, :, [0, 1, 2, 7, 8, 9]] = rng.uniform(-0.01, 0.01, (EP_STEPS, B, 6))
    return mem, goals, W


def _fossen(m, mass=None):
    auv = rexrov2() if mass is None else dict(rexrov2(), mass=mass)
    return m.Handle(k=64, tau=4, s_dim=13, a_dim=6, dt=0.1, sigma=np.eye(6), goal=np.zeros(13), auv=auv)


@pytest.mark.parametrize("plants", ["own", "shared", "per-member"])
def test_episodes_equal_the_lone_handles_episodes(m, plants):
    """two calls of two steps (the second continues where the first stopped), a goal per step, a disturbance: X, U, C bit for bit"""
    mem, goals, W = _episode_members()
    hb = N.make_batch(m, EP, mem)
    lone = [N.make_lone(m, EP, mem, i) for i in range(EP["B"])]
    ps = [] if plants == "own" else [_fossen(m)] if plants == "shared" else [_fossen(m, mass) for mass in (1500.0, 1862.87, 2300.0)]
    kb = {} if not ps else dict(plant=ps[0] if len(ps) == 1 else ps)
    xb, xl = mem["X"], [mem["X"][i] for i in range(EP["B"])]
    for call in range(2):
        sl = slice(2 * call, 2 * call + 2)
        Xb, Ub, Cb = hb.run_episode(xb, 2, goals[sl], W[sl], **kb)
        assert np.isfinite(Xb).all() and np.isfinite(Cb).all()
        for i, h in enumerate(lone):
            kl = {} if not ps else dict(plant=ps[0] if len(ps) == 1 else ps[i])
            Xl, Ul, Cl = h.run_episode(xl[i], 2, goals[sl, i], W[sl, i], **kl)
            msg = "member %d call %d (%s)" % (i, call, plants)
            np.testing.assert_array_equal(Ub[:, i], Ul, err_msg="U " + msg)
            np.testing.assert_array_equal(Xb[:, i], Xl, err_msg="X " + msg)
            np.testing.assert_array_equal(Cb[:, i], Cl, err_msg="C " + msg)
            xl[i] = Xl[-1]
        xb = Xb[-1]
    if plants == "own":  # every member was stepped by its OWN network: members 0 and 1 from one state and control part ways
        assert hb.get_step_counter() == 4
    for h in lone + ps:
        h.close()
    hb.close()


# ---- 6. the learner bridge ------------------------------------------------------------------------------------------------------------
def test_load_learners_and_episode_fold(m):
    case = dict(EP, hid=16, nh=2, B=4)
    rng = np.random.default_rng(3)
    net = N.make_net(case, 21)
    weights = dict(W=net["W"], b=net["b"])
    norm = {k: net[k] for k in ("xmean", "xstd", "ymean", "ystd")}
    lb = m.LearnerBatch(weights, 4)
    n = 96
    lb.set_data(rng.standard_normal((n, 16)).astype(F32), (0.1 * rng.standard_normal((n, 13))).astype(F32))
    for i in range(4):
        lb.set_split(i, np.arange(i, n, 2), None)
    lb.train(2, np.array([1e-3, 3e-3, 1e-2, 3e-2], F32))
    B, H = 4, case["H"]
    G = np.tile(N.GOAL13, (B, 1)).astype(F32)
    X = np.tile(N.X0, (B, 1)).astype(F32)
    mem = dict(nets=[net] * 4, seeds=[3, 4, 5, 6], lams=[1.0] * 4, G=G, X=X, U0=np.zeros((B, H, 6), F32))
    hb = N.make_batch(m, case, mem)
    model = dict(kind="nnauv", s_dim=13, a_dim=6, **norm)
    hb.load_learners(lb, model)
    u = hb.next(X)
    for i in range(4):
        h = N.make_lone(m, case, dict(mem, nets=[dict(lb.get_weights(j), **norm) for j in range(4)]), i)
        np.testing.assert_array_equal(u[i], h.next(X[i]), err_msg="member %d" % i)
        h.close()
    assert np.abs(u[0] - u[3]).max() > 0  # the rates differ, so do the networks
    # episode_fold: the summed state cost of every member's closed-loop episode
    plant = _fossen(m)
    hb2 = N.make_batch(m, case, mem)
    ctl = N.make_batch(m, case, mem)
    nn = m.NNAUVModel(weights=net)
    nn.set_Xmean_Xstd(net["xmean"], net["xstd"])
    nn.set_Ymean_Ystd(net["ymean"], net["ystd"])
    cost = m.LearnerBase(nn).episode_fold(lb, ctl, plant, X[0], 3)
    hb2.load_learners(lb, model)
    _, _, Cs = hb2.run_episode(X, 3, plant=plant)
    assert cost.shape == (4,) and np.isfinite(cost).all()
    np.testing.assert_array_equal(cost, Cs.sum(0))
    for h in (hb, hb2, ctl, plant):
        h.close()
    lb.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def _create(m, arr, n=None):
    from mppi_tf_amd import _lib
    lib = _lib.load()
    h = _lib._H()
    st = lib.mppi_create_batch_learned(arr, len(arr) if n is None else n, C.byref(h))
    if h:
        lib.mppi_destroy(h)
    return st, lib.mppi_last_error(None).decode(), bool(h)


def _learned_configs(n, net, speed=False, **fields):
    from mppi_tf_amd import _lib

    def each(i, cfg, keep):
        desc, held = _lib._mlp_desc(net, 15 if speed else 16, 6 if speed else 13)
        keep += held
        cfg.model_kind, cfg.mlp = (_lib.MODEL_NN_AUV_SPEED if speed else _lib.MODEL_NN_AUV), C.pointer(desc)
        for key, v in fields.items():
            setattr(cfg, key, v)
    return raw_configs(n, 13, 6, k=128, tau=4, each=each)


def test_refusals_name_their_cause(m):
    from mppi_tf_amd import _lib as L
    from mppi_tf_amd import _lib
    case = N.CASES[0]
    net = N.make_net(case, 1)
    arr, keep = _learned_configs(2, net)
    assert _create(m, arr)[0] == L.OK
    # MPPI_ERR_UNSUPPORTED, each with the word that names it
    for fields, word in ((dict(model_kind=_lib.MODEL_MLP), "MLP"), (dict(model_kind=_lib.MODEL_POINT_MASS), "mppi_create_batch_configs"),
                         (dict(model_kind=_lib.MODEL_AUV), "mppi_create_batch_configs"), (dict(normalize_cost=1), "normalize_cost"),
                         (dict(flags=2), "MPPI_FLAG_MLP_BF16X3"), (dict(flags=4), "MPPI_FLAG_FP_CONTRACT"), (dict(shard_count=2), "shard_count")):
        arr, keep = _learned_configs(2, net, **fields)
        st, err, got = _create(m, arr)
        assert (st, got) == (L.ERR_UNSUPPORTED, False) and word in err, (fields, err)
        assert _lib.load().mppi_last_error(None).decode() == err  # mppi_last_error(NULL) after a failed create
    arr, keep = _learned_configs(1, net, k=64 * 1025)
    st, err, _ = _create(m, arr)
    assert st == L.ERR_UNSUPPORTED and "1024 tiles" in err
    # MPPI_ERR_INVALID_ARG
    lib = _lib.load()
    h = _lib._H()
    arr, keep = _learned_configs(2, net)
    assert lib.mppi_create_batch_learned(None, 2, C.byref(h)) == L.ERR_INVALID_ARG and "NULL" in lib.mppi_last_error(None).decode()
    assert lib.mppi_create_batch_learned(arr, 2, None) == L.ERR_INVALID_ARG
    st, err, _ = _create(m, arr, 0)
    assert st == L.ERR_INVALID_ARG and "n must be >= 1" in err
    arr[1].mlp = None
    st, err, _ = _create(m, arr)
    assert st == L.ERR_INVALID_ARG and "member 1" in err and "cfg.mlp" in err
    big, keep2 = _learned_configs(1, net, k=65536)
    st, err, _ = _create(m, big, None)
    assert st == L.OK
    # the network's shape is shared: named as the other shared fields are
    a2, k2 = _learned_configs(2, net)
    d2, held = _lib._mlp_desc(N.make_net(dict(case, hid=16), 2), 16, 13)
    a2[1].mlp = C.pointer(d2)
    st, err, _ = _create(m, a2)
    assert st == L.ERR_INVALID_ARG and "cfgs[1].mlp.widths" in err
    d3, held3 = _lib._mlp_desc(N.make_net(dict(case, nh=2), 2), 16, 13)
    a2[1].mlp = C.pointer(d3)
    st, err, _ = _create(m, a2)
    assert st == L.ERR_INVALID_ARG and "cfgs[1].mlp.n_layers" in err
    a3, k3 = _learned_configs(2, net)
    a3[1].tau = 5
    st, err, _ = _create(m, a3)
    assert st == L.ERR_INVALID_ARG and "cfgs[1].tau" in err


def test_n_times_k_too_large_is_refused(m):
    from mppi_tf_amd import _lib as L
    net = N.make_net(N.CASES[0], 1)
    arr, keep = _learned_configs(1, net, k=65536)
    big = (type(arr[0]) * 20000)(*([arr[0]] * 20000))
    st, err, got = _create(m, big)
    assert (st, got) == (L.ERR_INVALID_ARG, False) and "n * k too large" in err


def test_the_handle_refuses_what_a_batch_refuses(m):
    from mppi_tf_amd import _lib as L
    ci = 0
    case, mem = N.CASES[ci], N.members(ci)
    hb = N.make_batch(m, case, mem)
    lib = hb.lib
    x, u = mem["X"][0].copy(), np.zeros(6, F32)
    from mppi_tf_amd._lib import fp
    # the per-member entry points
    assert lib.mppi_next(hb.h, fp(x), 13, fp(u), 6) == L.ERR_UNSUPPORTED and "mppi_batch_" in lib.mppi_last_error(hb.h).decode()
    desc, held = __import__("mppi_tf_amd")._lib._mlp_desc(mem["nets"][0], 16, 13)
    assert lib.mppi_set_mlp(hb.h, C.byref(desc)) == L.ERR_UNSUPPORTED and "mppi_batch_set_mlp" in lib.mppi_last_error(hb.h).decode()
    assert lib.mppi_set_goal(hb.h, fp(x), 13) == L.ERR_UNSUPPORTED
    assert lib.mppi_set_sequence_filter(hb.h, 5, 3) == L.ERR_UNSUPPORTED and "mppi_set_sequence_filter" in lib.mppi_last_error(hb.h).decode()
    assert lib.mppi_set_transition_log(hb.h, 8) == L.ERR_UNSUPPORTED and "mppi_set_transition_log" in lib.mppi_last_error(hb.h).decode()
    # the tunings a batch refuses
    for key in ("mlp32_valu", "fused_step", "prelaunch", "force_tile_kernel"):
        with pytest.raises(m.MppiError) as e:
            hb.set_tuning(key, 1)
        assert e.value.status == L.ERR_UNSUPPORTED and key in str(e.value)
    # what serves any batch serves this one
    hb.set_action_limits([-1.0] * 6, [1.0] * 6)
    ul = hb.next(mem["X"])
    assert np.abs(hb.get_action_sequences()).max() <= 1.0 and np.abs(ul).max() <= 1.0
    hb.set_step_counter(7)
    assert hb.get_step_counter() == 7
    hb.profile_begin(2)
    hb.next(mem["X"])
    r, f, n = hb.profile_end()
    assert n == 1 and r > 0 and f > 0
    hb.close()
    # BatchHandle itself keeps refusing a learned model, and so does mppi_create_batch
    from batch_util import batch_with_mlp
    with pytest.raises(m.MppiError) as e:
        batch_with_mlp(m, dict(nnauv=mem["nets"][0]))
    assert e.value.status == L.ERR_UNSUPPORTED and "model NNAUV is not supported" in str(e.value)
    with pytest.raises(TypeError):
        m.BatchHandle(n=2, k=64, tau=4, s_dim=13, a_dim=6, nnauv=mem["nets"][0])
