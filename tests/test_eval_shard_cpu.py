"""The deal / pack / un-deal helpers of the sharded test pass (evaluate.shard_batches, pack_shard, undeal_shards; DESIGN.md
section 24) on CPU tensors: batch b goes to replica b % W, every replica packs its rows and per-batch losses into one
buffer of ceil(batches / W) slots, the rank-ordered concatenation of the buffers (what one all-gather returns) un-deals
into the single-process row order and batch losses, exactly."""
import pytest
import torch

CASES = [(45, 8, 1), (45, 8, 2), (45, 8, 4), (36, 36, 3), (5, 8, 2)]
WIDTH, K = 7, 4


def _ev():
    from multimodal_learning_amd import evaluate
    return evaluate


def _truth(n_rows, batch):
    g = torch.Generator().manual_seed(n_rows * 131 + batch)
    nb = -(-n_rows // batch)
    # no zero anywhere: a row or loss that came back from the padding would show
    return torch.rand(n_rows, WIDTH, generator=g) + 1.0, torch.rand(nb, K, generator=g) + 1.0


@pytest.mark.parametrize("n_rows,batch,W", CASES)
def test_every_batch_is_dealt_once_in_order(n_rows, batch, W):
    E = _ev()
    nb, slots = E.shard_slots(n_rows, batch, W)
    assert nb == -(-n_rows // batch) and slots == -(-nb // W)
    seen = {}
    for r in range(W):
        mine = E.shard_batches(n_rows, batch, r, W)
        assert [b for b, _, _ in mine] == list(range(r, nb, W)) and len(mine) <= slots
        for b, lo, hi in mine:
            assert lo == b * batch and hi == min(lo + batch, n_rows) and hi > lo
            seen[b] = (lo, hi)
    assert sorted(seen) == list(range(nb))
    assert [seen[b][0] for b in range(1, nb)] == [seen[b - 1][1] for b in range(1, nb)] and seen[nb - 1][1] == n_rows


def test_the_cases_include_an_idle_replica_and_a_partial_last_batch_off_rank_0():
    E = _ev()
    assert E.shard_batches(36, 36, 1, 3) == [] and E.shard_batches(36, 36, 2, 3) == []        # replicas with no batch
    assert E.shard_batches(5, 8, 1, 2) == [] and E.shard_batches(5, 8, 0, 2) == [(0, 0, 5)]    # a single partial batch
    assert E.shard_batches(45, 8, 1, 2)[-1] == (5, 40, 45)         # the partial batch is replica 1's last one
    assert E.shard_batches(45, 8, 1, 4)[-1] == (5, 40, 45) and len(E.shard_batches(45, 8, 2, 4)) == 1


@pytest.mark.parametrize("n_rows,batch,W", CASES)
def test_round_trip_through_an_in_process_gather(n_rows, batch, W):
    E = _ev()
    rows, losses = _truth(n_rows, batch)
    nb, slots = E.shard_slots(n_rows, batch, W)
    bufs = []
    for r in range(W):
        mine = E.shard_batches(n_rows, batch, r, W)
        buf = E.pack_shard([rows[lo:hi] for _, lo, hi in mine], [losses[b] for b, _, _ in mine], n_rows, batch, W,
                           like=(WIDTH, K, torch.device("cpu")))
        assert buf.dtype == torch.float32 and buf.dim() == 1 and buf.numel() == slots * batch * WIDTH + slots * K
        bufs.append(buf)
    gathered = torch.cat(bufs, 0)                    # all_gather_cat: rank-ordered
    got_rows, got_losses = E.undeal_shards(gathered, n_rows, batch, W, WIDTH, K)
    assert got_rows.shape == (n_rows, WIDTH) and got_losses.shape == (nb, K)
    assert got_rows.is_contiguous() and got_losses.is_contiguous()
    assert torch.equal(got_rows, rows) and torch.equal(got_losses, losses)
    # the padding is zero and nothing else is: the buffers hold exactly the rows and losses
    assert int((gathered != 0).sum()) == n_rows * WIDTH + nb * K


def test_a_wrong_deal_is_noticed():
    """Negative control: buffers concatenated in another rank order do not un-deal to the rows."""
    E = _ev()
    n_rows, batch, W = 45, 8, 2
    rows, losses = _truth(n_rows, batch)
    bufs = []
    for r in range(W):
        mine = E.shard_batches(n_rows, batch, r, W)
        bufs.append(E.pack_shard([rows[lo:hi] for _, lo, hi in mine], [losses[b] for b, _, _ in mine], n_rows, batch, W))
    got_rows, _ = E.undeal_shards(torch.cat(bufs[::-1], 0), n_rows, batch, W, WIDTH, K)
    assert not torch.equal(got_rows, rows)
