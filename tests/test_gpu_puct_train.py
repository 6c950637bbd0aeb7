"""The closed loop on one GPU: PUCT self-play on the current model, its records and root
visit rows collected on the device (training.selfplay_puct_device), the soft-target
dataset and the existing epochs (training.run_iteration(search="puct"))."""
import random

import numpy as np
import pytest
import torch

import puct_ref as R

pytestmark = pytest.mark.gpu


def _model(seed=7):
    from gzero import weights
    from neural_network import GomokuModel
    model = GomokuModel(device="cpu")
    model.model.load_state_dict(weights.init_state_dict(seed=seed))
    return model


def _replay(moves):
    """Play row-major moves from the empty board; returns (cells per ply, winner or 0, over)."""
    cells = [0] * 225
    before = []
    over, winner = False, 0
    for k, m in enumerate(moves):
        assert not over and cells[m] == 0, "illegal move in a record"
        before.append(tuple(cells))
        pl = 1 + k % 2
        cells[m] = pl
        if R.makes_five(cells, m, pl):
            over, winner = True, pl
        elif 0 not in cells or k + 1 >= 200:
            over = True
    return before, winner, over


def test_puct_collection_on_the_device():
    """4 games at 8 simulations, temp_plies 6, ids [12, 16): exactly those ids, sorted by
    (game id, ply), every game legal and played to its end, every visit row summing to
    the simulation count, zero on occupied cells and positive at the move played -- and
    the same records and rows as the host-side collection (training.selfplay)."""
    import training
    from gzero.boards import RECORD_DTYPE, words_to_cells
    from gzero.train import DeviceTrainer
    S, temp, n_games, base, seed = 8, 6, 4, 12, 11
    model = _model()
    DeviceTrainer(model)  # the model on the device, as run_iteration has it
    d, d_vis, n, st = training.selfplay_puct_device(n_games, num_simulations=S, seed=seed, game_id_base=base,
                                                    model=model, temp_plies=temp)
    assert d.is_cuda and d_vis.is_cuda and tuple(d.shape) == (n, 80) and tuple(d_vis.shape) == (n, 225)
    assert d_vis.dtype == torch.int16
    recs = np.frombuffer(d.cpu().numpy().tobytes(), RECORD_DTYPE)
    vis = d_vis.cpu().numpy().view(np.uint16)
    assert sorted(set(int(g) for g in recs["game_id"])) == list(range(base, base + n_games))
    keys = [(int(g), int(p)) for g, p in zip(recs["game_id"], recs["ply"])]
    assert keys == sorted(keys) and len(set(keys)) == n
    assert st["games"] == n_games and st["moves_played"] >= n
    cells = words_to_cells(recs["black"], recs["white"])
    for gid in range(base, base + n_games):
        at = np.flatnonzero(recs["game_id"] == gid)
        moves = [int(m) for m in recs["move"][at]]
        assert [int(p) for p in recs["ply"][at]] == list(range(len(moves)))
        before, winner, over = _replay(moves)
        assert over, gid
        players = [1 + k % 2 for k in range(len(moves))]
        assert [int(p) for p in recs["player"][at]] == players
        assert [int(z) for z in recs["z"][at]] == [0 if winner == 0 else (1 if pl == winner else -1) for pl in players]
        for k, (i, m) in enumerate(zip(at, moves)):
            assert tuple(int(c) for c in cells[i]) == before[k]
            assert int(vis[i].sum()) == S
            assert not vis[i][np.array(before[k]) != 0].any()
            assert vis[i][m] > 0
    # the host-side collection of the same games
    replay, hst = training.selfplay(n_games, num_simulations=S, seed=seed, game_id_base=base, model=model,
                                    search="puct", temp_plies=temp, plies_per_step=4)
    assert len(replay) == n and hst["visits"].dtype == np.uint16 and hst["visits"].shape == (n, 225)
    assert replay.move_indices == [int(m) for m in recs["move"]]
    assert np.array_equal(hst["visits"], vis)
    with pytest.raises(ValueError):
        training.selfplay(1, model=None, search="puct")
    with pytest.raises(ValueError):
        training.selfplay(1, model=model, search="puct", planner_steps=2)


def test_run_iteration_puct_one_gpu():
    """Iteration 3 with 4 games per iteration (ids 12..15) at 8 simulations, batch 32, one
    epoch: the records are the plies of those games, the samples the 35 % augmented set,
    the losses finite, and every weight tensor moved."""
    import training
    from gzero.train import DeviceTrainer
    model = _model()
    trainer = DeviceTrainer(model)
    before = [p.detach().clone() for p in model.model.parameters()]
    random.seed(123)
    torch.manual_seed(456)
    res = training.run_iteration(model, trainer, 3, games_per_iteration=4, num_simulations=8, batch_size=32,
                                 epochs=1, seed=11, search="puct", verbose=False)
    n = res["records"]
    # the plies played: the same games again (the model's weights at the start, ids 12..15)
    again = _model()
    DeviceTrainer(again)
    _, _, want, _ = training.selfplay_puct_device(4, num_simulations=8, seed=11, game_id_base=12, model=again,
                                                  temp_plies=8)
    assert n == want and n >= 4 * 9
    assert res["samples"] == n + 8 * max(1, int(0.35 * n))
    assert np.isfinite(res["train_loss"]) and np.isfinite(res["val_loss"])
    assert all(not torch.equal(a, b) for a, b in zip(before, model.model.parameters()) if a.dim() > 1)
    with pytest.raises(ValueError):
        training.run_iteration(model, trainer, 0, search="mcts")
