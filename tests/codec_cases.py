"""Chosen Reed-Solomon error patterns for the by-word step kernels, and a CPU reference of the step.  CPU only; imported by
test_codec_cases_host.py and test_gpu_byword_codec.py.

  batch(nsym, n)
      One batch of words per (nsym, n) of CASES: random messages (bit 0 = 0) encoded by the C oracle, then corrupted in chosen BYTES:
      e = 0 .. min(n, t + 2) byte errors (t = nsym // 2), three words per e on the special positions {0, k-1, k, n-1, 63, 64, n//2}
      (lane-stride wrap of the `p += 64` loops, seam of the two ballots, message/parity seam, both ends) and three on random
      positions (and six more clean words), then words whose errors sit in the parity bytes only.  Error values are random and
      non-zero, one in four a single bit; at byte 0 their MSB is clear, so bit 0 of every word stays 0 (symbol 0 is decided 0 by
      every detector: quirk Q1).
  clean_channel(words, sigma)
      The words over the static time-decay channel (isi_awgn_kernel's anti-causal 4-tap convolution, in float64).  Without noise
      the Viterbi detector returns the word as sent, so the step kernels can be handed any of the patterns above.
  reference_step(dec, tx_msg, nsym, pilot)
      What one block step of the by-word evaluation computes from the detector's decisions (trainer.py:292-324 of the reference),
      from the C oracle's codec alone.
"""
import functools

import numpy as np

import meta_viterbinet_amd as mvn
import oracle

L = 4  # memory length of the 16-state trellis
NSYMS = tuple(range(1, 9))
SNR_VNET_DB = 40.0
SIGMA_VNET = 10.0 ** (-SNR_VNET_DB / 20.0)


# Clean words per batch beyond the six of e = 0: the trained ViterbiNet flips a few bits of a batch even at 40 dB, which turns about a
# third of the clean words into words with an error; with these the ViterbiNet table keeps its floor of clean words too.
EXTRA_CLEAN = 6


def lengths(nsym):
    """Codeword lengths n (bytes) of one nsym: the shortest code, the goldens' 17, and both sides of 64 and of 128."""
    return (nsym + 1, 17, 63, 64, 65, 127, 128)


CASES = tuple((nsym, n) for nsym in NSYMS for n in lengths(nsym))


def special_positions(nsym, n):
    """{0, k-1, k, n-1, 63, 64, n//2} inside [0, n), without repeats; 63 and 64 next to each other."""
    k = n - nsym
    out = []
    for p in (0, k - 1, 63, 64, k, n - 1, n // 2):
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


def unpack(rows):
    """uint8 [R, n] -> fp32 bits [R, 8 n], MSB first (np.unpackbits order)."""
    return np.unpackbits(np.ascontiguousarray(rows, dtype=np.uint8), axis=1).astype(np.float32)


def pack(bits):
    return np.packbits(np.asarray(bits).astype(np.uint8), axis=1)


def _error_value(rng, p):
    """Random and non-zero, MSB clear at byte 0; one value in four is a single bit (a lone wrong message bit is the smallest error
    count at which the label word is the detection)."""
    bits = 7 if p == 0 else 8
    if rng.randint(4) == 0:
        return 1 << int(rng.randint(bits))
    return int(rng.randint(1, 1 << bits))


@functools.lru_cache(maxsize=None)
def batch(nsym, n):
    """dict: msg [R, 8k] fp32 (what was transmitted), cw [R, 8n] its codeword, word [R, 8n] the corrupted codeword, pos: per word the
    tuple of corrupted byte positions, parity_only: bool [R]."""
    k, t = n - nsym, nsym // 2
    rng = np.random.RandomState(7919 * nsym + n)
    spec = special_positions(nsym, n)
    patterns, parity_only = [], []
    turn = (nsym + n) % len(spec)  # where the rotation through the special positions starts: differs from batch to batch
    for e in range(0, min(n, t + 2) + 1):
        for j in range(3):
            if e >= 2 and j == 0 and 63 in spec and 64 in spec:
                turn = spec.index(63)  # one word per e with errors on both sides of the seam
            pos = [spec[(turn + i) % len(spec)] for i in range(min(e, len(spec)))]
            turn = (turn + len(pos)) % len(spec)
            rest = [p for p in range(n) if p not in pos]
            pos += [int(p) for p in rng.choice(rest, e - len(pos), replace=False)] if e > len(pos) else []
            patterns.append(tuple(pos))
            parity_only.append(False)
        for j in range(3 if e else 3 + EXTRA_CLEAN):
            patterns.append(tuple(int(p) for p in rng.choice(n, e, replace=False)))
            parity_only.append(False)
    for e in range(1, min(nsym, t + 2) + 1):
        patterns.append(tuple(int(p) for p in k + rng.choice(nsym, e, replace=False)))
        parity_only.append(True)
    R = len(patterns)
    msg = unpack(rng.randint(0, 256, (R, k)))
    msg[:, 0] = 0.0
    cw = oracle.rs_encode_bits(msg, nsym)
    rows = pack(cw)
    for r, pos in enumerate(patterns):
        for p in pos:
            rows[r, p] ^= _error_value(rng, p)
    word = unpack(rows)
    assert np.all(word[:, 0] == 0)
    return dict(nsym=nsym, n=n, k=k, msg=msg, cw=cw, word=word, pos=patterns, parity_only=np.array(parity_only))


@functools.lru_cache(maxsize=None)
def channel():
    """The static time-decay taps [1, 4] (float64) and the Viterbi detector's state priors for them [1, 16] (float32)."""
    h = mvn.estimate_channel(L, 0.2, "time_decay", fading=False, index=0)
    va = mvn.VADetector(16, L, 8, 1, "ISI_AWGN", 0, False, 1, {"train": "time_decay", "val": "time_decay"})
    pri = np.ascontiguousarray(va.compute_state_priors(h).cpu().numpy().T, dtype=np.float32)
    return np.asarray(h, np.float64), pri


def clean_channel(words, sigma, seed=0):
    """y[t] = sum_i h[L-1-i] (1 - 2 c[t+i]) + sigma w[t] in float64 (c zero-padded by L; w standard normal from `seed`), as float32."""
    c = np.asarray(words, np.float64)
    B, T = c.shape
    h = channel()[0][0]
    s = np.concatenate([1.0 - 2.0 * c, np.ones((B, L))], axis=1)
    y = np.zeros((B, T))
    for i in range(L):
        y += h[L - 1 - i] * s[:, i:i + T]
    if sigma:
        y += sigma * np.random.RandomState(seed).standard_normal((B, T))
    return y.astype(np.float32)


def vnet_rx(nsym, n):
    """The batch's words at 40 dB, the ViterbiNet step's input (fixed noise per batch)."""
    return clean_channel(batch(nsym, n)["word"], SIGMA_VNET, seed=104729 * nsym + n)


def reference_step(dec, tx_msg, nsym, pilot):
    """One block step for every row (trainer.py:292-324): data block: msg = decode(dec), nerr = #(msg != tx), enc = encode(msg),
    label word = dec if nerr > 0 else enc; pilot block: enc = label word = encode(tx), nerr = 0, no msg.  labels: the label word's
    trellis states [R, T].  status: the oracle's decoder status (None on a pilot)."""
    tx_msg = np.ascontiguousarray(tx_msg, dtype=np.float32)
    if pilot:
        enc = oracle.rs_encode_bits(tx_msg, nsym)
        msg, status, lw = None, None, enc
        nerr = np.zeros(tx_msg.shape[0], np.int32)
    else:
        dec = np.ascontiguousarray(dec, dtype=np.float32)
        msg, status = oracle.rs_decode_bits(dec, nsym, want_status=True)
        nerr = (msg != tx_msg).sum(axis=1).astype(np.int32)
        enc = oracle.rs_encode_bits(msg, nsym)
        lw = np.where((nerr > 0)[:, None], dec, enc).astype(np.float32)
    labels = oracle.calculate_states(L, lw).reshape(lw.shape).astype(np.int32)
    return dict(msg=msg, nerr=nerr, enc=enc, label_word=lw, labels=labels, status=status)


def outcome_counts(dec, b):
    """How the oracle's decoder ends on the detected words `dec` of batch b: words without a byte error, words with 1..t byte errors
    decoded back to the message, words ending in status 1, words with status 0 and a wrong message, status 2, and words with at
    most t byte errors that did not decode to the message.  The byte errors are counted in `dec` itself."""
    ref = reference_step(dec, b["msg"], b["nsym"], False)
    nbytes = (pack(dec) != pack(b["cw"])).sum(axis=1)
    t = b["nsym"] // 2
    ok = ref["nerr"] == 0
    return dict(clean=int(np.sum(nbytes == 0)), corrected=int(np.sum((nbytes >= 1) & (nbytes <= t) & ok & (ref["status"] == 0))),
                status1=int(np.sum(ref["status"] == 1)), wrong0=int(np.sum((ref["status"] == 0) & ~ok)),
                status2=int(np.sum(ref["status"] == 2)), failed_within_t=int(np.sum((nbytes <= t) & ~ok)))


FLOORS = dict(clean=30, corrected=40, status1=40, wrong0=40)  # per nsym, summed over its n


def g7_weights(golden):
    g7 = golden("g7_by_word")
    return [np.ascontiguousarray(g7[f"w{i}"], dtype=np.float32) for i in range(6)]
