"""bench.py's timed path on the GPU, at a small size: what --dump-outputs
writes is the dst the last timed launch wrote, and it is the same in every
run although the clock prewarm's launch count is not.
"""
import types

import numpy as np
import pytest

import bench
import oracle

COUNT = (1 << 18) + 3          # ragged: not a multiple of the kernel's tile
SEED, W, K, NSETS, SAMPLE = 77, 3, 5, 2, 4096


@pytest.mark.gpu
def test_timed_combine_returns_the_last_steps_dst_in_every_run():
    """W warmup + K timed launches rotate over NSETS pairs from index 0 each,
    so the last timed launch writes pair (K-1) % NSETS, which has then taken
    a known number of float adds of its src (5 here; the other pair 3).  The
    sample must equal the oracle's result of exactly those adds on the seeded
    buffers — with a prewarm (whose launches are undone by reseed_dst),
    without one, and with the isolated-median launches that follow the
    sample."""
    import torch
    torch.cuda.set_device(0)
    dev, stream = torch.device("cuda", 0), torch.cuda.current_stream()

    def run(prewarm_s, isolated):
        args = types.SimpleNamespace(prewarm_s=prewarm_s, warmup=W, steps=K)
        return bench.timed_combine(dev, stream, COUNT, SEED, args, 1, sample=SAMPLE,
                                   isolated=isolated, nsets=NSETS)

    a, b, c = run(0.05, False), run(0.05, True), run(0.0, False)
    assert a["prewarm"] > 0 and b["prewarm"] > 0 and c["prewarm"] == 0
    assert a["kern_med"] is None and b["kern_med"] > 0 and a["nsets"] == NSETS

    last = (K - 1) % NSETS
    adds = sum(i % NSETS == last for i in range(W)) + sum(i % NSETS == last for i in range(K))
    assert adds == 5
    dst, src = bench.make_buffers(dev, SEED, COUNT, NSETS)[last]
    want, s = dst.cpu().numpy(), src.cpu().numpy()
    for _ in range(adds):
        oracle.write(bench.FI_SUM, bench.FI_FLOAT, want, s)
    want = want[bench.sample_index(COUNT, SAMPLE)]
    for r in (a, b, c):
        got = r["last_out"]
        assert got.dtype == np.float32 and got.shape == (SAMPLE,)
        assert got.tobytes() == want.tobytes()
