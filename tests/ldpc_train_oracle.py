"""A numpy restatement of the draws of fgnn_ldpc_sample_rng (include/fgnn_hip_ldpc_train.h; csrc/ldpc_datapath.hip, the DRAW prologue
of ldpc_features_kernel), built on oracle/fgnn_oracle.py as it is: ``philox4x32``, ``ldpc_encode``, ``philox_channel_draws``,
``ldpc_channel``.  Not a test module.

Per codeword b one Philox4x32-10 block, key = seed, counter = (b lo, b hi | 0x80000000, step lo, step hi):
    message bit c = bit c of word 0 (c < 32) / bit c - 32 of word 1;  SNR class = word 2 * n_snr >> 32;  burst class = word 3 * n_sigma >> 32.
"""
import numpy as np

import fgnn_oracle as O

K = 48
SNR_CHOICES = (0, 1, 2, 3, 4)               # LdpcDataPath.snr_db_choices (ldpc_dataset.py:216)
SIGMA_CHOICES = (0, 1, 2, 3, 4, 5)          # LdpcDataPath.sigma_b_choices (ldpc_dataset.py:212)


def sample_draws(B, seed, step, n_snr=len(SNR_CHOICES), n_sigma=len(SIGMA_CHOICES), k=K):
    """(messages [B, k] uint8, SNR class index [B] int64, burst class index [B] int64) of batch ``step`` under ``seed``."""
    b = np.arange(B, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    counter = np.stack([b & m32, (b >> np.uint64(32)) | np.uint64(0x80000000), np.full_like(b, np.uint64(step & 0xFFFFFFFF)),
                        np.full_like(b, np.uint64((step >> 32) & 0xFFFFFFFF))], axis=-1)
    r = O.philox4x32(counter, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).astype(np.uint64)
    word = r[:, 0] | (r[:, 1] << np.uint64(32))
    s = ((word[:, None] >> np.arange(k, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    snr_idx = ((r[:, 2] * np.uint64(n_snr)) >> np.uint64(32)).astype(np.int64)
    sigma_idx = ((r[:, 3] * np.uint64(n_sigma)) >> np.uint64(32)).astype(np.int64)
    return s, snr_idx, sigma_idx


def sample_batch(G, B, seed, step, snr_choices=SNR_CHOICES, sigma_choices=SIGMA_CHOICES, rho=0.05):
    """The sampler's batch restated: cw [B, 96] uint8, snr_db [B] f32, sigma_b [B] f32, and y [B, 96] float64 — ``ldpc_channel`` on
    the restated draws of the channel kernel at the same (seed, step) (``philox_channel_draws``)."""
    s, i_snr, i_sigma = sample_draws(B, seed, step, len(snr_choices), len(sigma_choices), np.asarray(G).shape[1])
    cw = O.ldpc_encode(G, s)
    snr = np.asarray(snr_choices, np.float32)[i_snr]
    sb = np.asarray(sigma_choices, np.float32)[i_sigma]
    z1, u, z2 = (a.reshape(cw.shape) for a in O.philox_channel_draws(cw.size, seed, step))
    y = O.ldpc_channel(cw, snr, sb, np.float32(rho), z1, u, z2)
    return cw, snr, sb, y
