"""The multi-rank read of the device episode windows on CPU: two gloo ranks each hold their window buffers
(metrics.EpisodeMetrics.buffers, [parts, words] int64) and distributed.gather_windows must hand every rank the
concatenation in rank order -- global bin order under distributed.shard -- with one all_gather."""
import os
import socket

import torch
import torch.multiprocessing as mp

import irbpp_amd  # noqa: F401
from irbpp_amd import distributed as D
from irbpp_amd.metrics import window_words

PARTS, W, H = 2, 10, 8


def _buffers(rank):
    words = window_words(W, H)
    return torch.arange(PARTS * words, dtype=torch.int64).view(PARTS, words) + 1_000_000 * (rank + 1)


def _worker(rank, world, port, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    D.init_from_env("gloo")
    out = D.gather_windows(_buffers(rank))
    ret[rank] = out.clone()
    torch.distributed.destroy_process_group()


def test_gather_windows_in_rank_order():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, ret), nprocs=2, join=True)
    want = torch.cat([_buffers(0), _buffers(1)])
    for r in range(2):
        assert ret[r].shape == (2 * PARTS, window_words(W, H))
        assert torch.equal(ret[r], want)


def test_gather_windows_without_a_process_group_is_the_identity():
    b = _buffers(0)
    assert D.gather_windows(b) is b
