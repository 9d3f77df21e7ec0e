"""CPU tests of the LSTM-VAE training path's yardstick (tests/vae_yardstick.py) and parameter table (no GPU).

- Without dropout the yardstick is oracle.traj2z / oracle.lstm_decode / oracle.vae_loss to 1e-12 in float64, an all-ones mask changes
  nothing, and on the encoder / decoder fixtures it meets the values recorded from the reference with the oracle's own bars.
- Its float64 autograd agrees with central finite differences, with dropout masks, through the whole step (encode -> reparametrise ->
  decode -> loss) on entries of every tensor kind of both LSTMs, the heads and cond2hidden, and on x6, cond and (the decoder alone) z.
- The flat parameter table of the C-ABI (cld_vae_param_info, no handle needed) holds LSTMVAE's 26 tensors in state_dict order with their
  shapes, 136,458 values, at aligned offsets.
"""
import os

import numpy as np
import torch

import vae_yardstick as Y
from cld_amd import synth
from oracle import cld_oracle as O

ENTRIES = [
    ("lstm_enc.lstm.weight_ih_l0", (5, 3)), ("lstm_enc.lstm.weight_hh_l0", (200, 17)), ("lstm_enc.lstm.bias_ih_l0", (70,)),
    ("lstm_enc.lstm.bias_hh_l0", (140,)), ("lstm_enc.lstm.weight_ih_l1", (150, 40)), ("lstm_enc.lstm.weight_hh_l1", (30, 63)),
    ("lstm_enc.lstm.bias_ih_l1", (9,)), ("lstm_enc.lstm.bias_hh_l1", (130,)),
    ("lstm_enc.cond2hidden.weight", (9, 100)), ("lstm_enc.cond2hidden.bias", (33,)),
    ("mu.weight", (2, 10)), ("mu.bias", (3,)), ("logvar.weight", (1, 50)), ("logvar.bias", (0,)),
    ("lstm_dec.lstm.weight_ih_l0", (100, 2)), ("lstm_dec.lstm.weight_hh_l0", (250, 5)), ("lstm_dec.lstm.bias_hh_l0", (12,)),
    ("lstm_dec.lstm.weight_ih_l1", (64, 60)), ("lstm_dec.lstm.weight_hh_l1", (190, 8)), ("lstm_dec.lstm.bias_ih_l1", (201,)),
    ("lstm_dec.cond2hidden.weight", (40, 255)), ("lstm_dec.cond2hidden.bias", (7,)),
    ("lstm_dec.hid2act.weight", (1, 20)), ("lstm_dec.hid2act.bias", (0,)),
]


def _w(dtype=torch.float64):
    return {k: torch.tensor(v, dtype=dtype) for k, v in Y.weights(2).items()}


def _inputs(B, seed=1):
    x6 = torch.from_numpy(synth.normal(seed, "vae_x6", (B, 52, 6))).double() * 3.0
    z = torch.from_numpy(synth.normal(seed, "vae_z", (B, 52, 4))).double() * 2.0
    cond = torch.from_numpy(synth.make_inputs(B, seed)["cond_feat"]).double()
    noise = torch.from_numpy(synth.normal(seed, "vae_noise", (B, 52, 4))).double()
    return x6, z, cond, noise


def test_yardstick_without_dropout_is_the_oracle():
    w = _w()
    x6, z, cond, noise = _inputs(3)
    mu, lv = Y.encode(w, x6, cond)
    _, muo, lvo = O.traj2z(w, x6, cond, noise)
    assert float((mu - muo).abs().max()) <= 1e-12 and float((lv - lvo).abs().max()) <= 1e-12
    act = Y.decode(w, z, cond)
    assert float((act - O.lstm_decode(w, z, cond)).abs().max()) <= 1e-12
    ones = torch.ones(3, 52, 64, dtype=torch.float64)
    assert torch.equal(Y.encode(w, x6, cond, ones)[0], mu) and torch.equal(Y.decode(w, z, cond, ones), act)
    got, ref = torch.stack(Y.vae_loss(x6, act, mu, lv, 0.3)), torch.stack(O.vae_loss(x6, act, mu, lv, 0.3))
    assert float((got - ref).abs().max()) <= 1e-12


def test_yardstick_meets_the_reference_goldens(golden):
    meta, g = golden("encode")
    B = meta["B"]
    fut = synth.make_future(B, meta["in_seed"])
    x6s = O.state_to_state_and_action(torch.from_numpy(fut["target_positions"]), torch.from_numpy(fut["target_yaws"]),
                                      torch.from_numpy(fut["curr_speed"]), scaled=True)
    cond = torch.from_numpy(synth.make_inputs(B, meta["in_seed"])["cond_feat"])
    nz = torch.from_numpy(synth.normal(meta["noise_seed"], "enc_noise", (B, 52, 4)))
    mu, lv = Y.encode(O.to_torch(synth.make_encoder_weights(meta["w_seed"])), x6s, cond)
    for got, k in ((mu + nz * torch.exp(0.5 * lv), "z"), (mu, "mu"), (lv, "logvar")):
        assert np.abs(got.numpy() - g[k]).max() <= 1e-5, k
    meta, g = golden("decode")
    B = meta["B"]
    cond = torch.from_numpy(synth.make_inputs(B, meta["in_seed"])["cond_feat"])
    z = torch.from_numpy(synth.normal(meta["in_seed"], "dec_z", (B, 52, 4)))
    act = Y.decode(O.to_torch(synth.make_decoder_weights(meta["w_seed"])), z, cond)
    assert np.abs(act.numpy() - g["act_small"]).max() <= 2e-6


def _fd_check(checks, loss, h=1e-5):
    for g, tensor, idx in checks:
        old = float(tensor[idx])
        tensor[idx] = old + h
        fp = loss()
        tensor[idx] = old - h
        fm = loss()
        tensor[idx] = old
        fd = (fp - fm) / (2 * h)
        assert abs(float(g) - fd) <= 1e-8 + 1e-6 * abs(fd), (idx, float(g), fd)


def test_fp64_autograd_matches_finite_differences_with_dropout():
    B = 2
    w = _w()
    x6, z, cond, noise = _inputs(B)
    masks = tuple(torch.from_numpy(Y.mask(1, n, B)).double() for n in ("fd_mask_enc", "fd_mask_dec"))
    assert 0 < float((masks[0] == 0).double().mean()) < 0.5
    wg = {k: v.clone().requires_grad_(True) for k, v in w.items()}
    xg, cg = x6.clone().requires_grad_(True), cond.clone().requires_grad_(True)
    Y.step_loss(wg, xg, cg, noise, 0.3, masks)[0].backward()
    checks = [(wg[k].grad[idx], w[k], idx) for k, idx in ENTRIES]
    checks += [(xg.grad[1, 30, 2], x6, (1, 30, 2)), (xg.grad[0, 51, 5], x6, (0, 51, 5)), (xg.grad[1, 0, 4], x6, (1, 0, 4)),
               (cg.grad[0, 17], cond, (0, 17))]
    _fd_check(checks, lambda: float(Y.step_loss(w, x6, cond, noise, 0.3, masks)[0]))
    # z: the decoder alone, for a fixed cotangent of act
    d = torch.from_numpy(synth.normal(1, "fd_dact", (B, 52, 2))).double()
    zg = z.clone().requires_grad_(True)
    (Y.decode(w, zg, cond, masks[1]) * d).sum().backward()
    _fd_check([(zg.grad[1, 10, 3], z, (1, 10, 3)), (zg.grad[0, 51, 0], z, (0, 51, 0))],
              lambda: float((Y.decode(w, z, cond, masks[1]) * d).sum()))


def test_parameter_table_is_the_lstmvae_state_dict():
    from cld_amd import _lib
    from cld_amd.engine import vae_param_table
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    table, nflat = vae_param_table(lib, None)
    ref = Y.weights(0)
    assert [n for n, *_ in table] == list(ref)
    assert len(table) == 26 and sum(n for _, _, n, _ in table) == 136458
    end = 0
    for name, off, n, shape in table:
        assert off % 64 == 0 and off >= end
        assert shape == ref[name].shape and n == ref[name].size
        end = off + n
    assert nflat >= end
    assert lib.cld_vae_param_info(None, 26, None, None, None, None, None) == -1
    assert lib.cld_vae_tape_bytes(None, 0, 3) == 3 * lib.cld_vae_tape_bytes(None, 1, 1) == 3 * 173568
    assert lib.cld_vae_tape_bytes(None, 2, 3) == 0 and lib.cld_vae_tape_bytes(None, 0, 0) == 0
    assert lib.cld_vae_train_workspace_bytes(None, 0) == 0 < lib.cld_vae_train_workspace_bytes(None, 1)
