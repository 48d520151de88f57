"""A numpy restatement of fgnn_ldpc_sample_rng_words (include/fgnn_hip_ldpc_code.h; csrc/ldpc_code.hip) for any code, and the decoder
model of any code from the oracle's parts — built on oracle/fgnn_oracle.py as it is.  Not a test module.

Philox4x32-10, key = seed.  Block j of codeword b: counter (b lo, 0x80000000 | j, step lo, step hi).  Block 0: words 0, 1 = message
word 0, word 2 -> SNR class, word 3 -> burst class.  Block j >= 1: words 0, 1 = message word 2j - 1, words 2, 3 = message word 2j
(low 32 bits first).  Message bit c = bit c % 64 of message word c // 64; only the first K bits are used.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import fgnn_oracle as O

SNR_CHOICES = (0, 1, 2, 3, 4)               # LdpcDataPath.snr_db_choices
SIGMA_CHOICES = (0, 1, 2, 3, 4, 5)          # LdpcDataPath.sigma_b_choices


def sample_draws(B, seed, step, K, n_snr=len(SNR_CHOICES), n_sigma=len(SIGMA_CHOICES)):
    """(messages [B, K] uint8, SNR class index [B] int64, burst class index [B] int64) of batch ``step`` under ``seed``."""
    W = -(-K // 64)
    b = np.arange(B, dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    words = np.zeros((B, W), np.uint64)
    snr_idx = sigma_idx = None
    for j in range(1 + W // 2):
        counter = np.stack([b & np.uint64(0xFFFFFFFF), np.full_like(b, np.uint64(0x80000000 | j)),
                            np.full_like(b, np.uint64(step & 0xFFFFFFFF)), np.full_like(b, np.uint64((step >> 32) & 0xFFFFFFFF))], axis=-1)
        r = O.philox4x32(counter, key).astype(np.uint64)
        lo, hi = r[:, 0] | (r[:, 1] << np.uint64(32)), r[:, 2] | (r[:, 3] << np.uint64(32))
        if j == 0:
            words[:, 0] = lo
            snr_idx = ((r[:, 2] * np.uint64(n_snr)) >> np.uint64(32)).astype(np.int64)
            sigma_idx = ((r[:, 3] * np.uint64(n_sigma)) >> np.uint64(32)).astype(np.int64)
        else:
            words[:, 2 * j - 1] = lo
            if 2 * j < W:
                words[:, 2 * j] = hi
    c = np.arange(K)
    s = ((words[:, c // 64] >> (c % 64).astype(np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    return s, snr_idx, sigma_idx


def sample_batch(G, B, seed, step, snr_choices=SNR_CHOICES, sigma_choices=SIGMA_CHOICES, rho=0.05):
    """The sampler's batch restated for the code with generator G [P, K]: cw [B, N] uint8, snr_db [B] f32, sigma_b [B] f32 and
    y [B, N] float64 — ``ldpc_channel`` on the restated draws of the channel kernel at the same (seed, step)."""
    s, i_snr, i_sigma = sample_draws(B, seed, step, np.asarray(G).shape[1], len(snr_choices), len(sigma_choices))
    cw = O.ldpc_encode(G, s)
    snr = np.asarray(snr_choices, np.float32)[i_snr]
    sb = np.asarray(sigma_choices, np.float32)[i_sigma]
    z1, u, z2 = (a.reshape(cw.shape) for a in O.philox_channel_draws(cw.size, seed, step))
    return cw, snr, sb, O.ldpc_channel(cw, snr, sb, np.float32(rho), z1, u, z2)


@functools.lru_cache(maxsize=None)
def gallager(n, dv, dc, seed):
    """The test codes, built once per process."""
    from fgnn_amd.ldpc_code import LdpcCode
    return LdpcCode.gallager(n, dv, dc, seed)


def ldpc_model(sd, n_msg, node_feature, hop_feature, nn_idx_f2v, nn_idx_v2f, efeature_f2v, efeature_v2f, *, nedge_type=4, training=False):
    """``LDPCModel.forward`` for any code from ``O.factor_nn`` and the model's state dict: ``O.ldpc_model`` with the residual added
    and the first ``n_msg`` (not N // 2) logits kept.  Returns (logits [B, n_msg], snr [B, 1]); train mode updates ``sd``'s running
    statistics as the oracle does."""
    B, nvar = node_feature.shape[0], node_feature.shape[2]
    edge_mlp = lambda p, ef: O.conv1x1(sd, p + '2.', torch.relu(O.conv1x1(sd, p + '0.', ef)))
    res, hops = O.factor_nn(
        sd, 'main.', node_feature, [hop_feature, node_feature[:, 0, :, :].reshape(B, nvar, 1, 1)],
        [nn_idx_f2v, sd['hnn_idx_f2v'].repeat(B, 1, 1)], [nn_idx_v2f, sd['hnn_idx_v2f'].repeat(B, 1, 1)],
        [edge_mlp('emodel_f2v.', efeature_f2v), sd['hetype_f2v'].repeat(B, 1, 1, 1)],
        [edge_mlp('emodel_v2f.', efeature_v2f), sd['hetype_v2f'].repeat(B, 1, 1, 1)],
        dims=O.LDPC_DIMS, netypes=[nedge_type, 1], skip_link=O.LDPC_SKIP, aggregator='max', training=training)
    res = (res + node_feature[:, :1, :, :]).reshape(B, nvar)
    p = 'nhop_regressor.'
    h = F.linear(hops[1].reshape(B, -1), sd[p + '0.weight'], sd[p + '0.bias'])
    h = torch.relu(O.batch_norm(h, sd, p + '1.', training))
    h = torch.relu(F.linear(h, sd[p + '3.weight'], sd[p + '3.bias']))
    h = torch.relu(F.linear(h, sd[p + '5.weight'], sd[p + '5.bias']))
    return res[:, :n_msg].contiguous(), h
