"""mmf_amd.clip_training's study (sample_trials, ClipProjectionTuner, run_hyperparameter_tuning, --tune) without a
GPU: on a CPU stand-in engine whose *_trials methods run tests/clip_train_refs.py's float32 epoch / evaluate per
trial, the tuner must give every trial the history ClipProjectionTrainer.fit gives for it alone -- value for value:
both go through the same restatement -- and follow the study's rule (the validation loss at the best-accuracy
epoch, minimised, ties to the lower trial number, inf for a trial whose loss turned non-finite)."""
import copy
import types

import numpy as np
import pytest
import torch

import mmf_amd.clip_training as CT
from tests import clip_train_refs as R
from tests.test_clip_train_refs_cpu import _clip_state, _CpuEngine, _Detective, _images, _StubForensics

NAN = float("nan")


class _TrialsEngine(_CpuEngine):
    """Engine.clip_train_epoch_trials / clip_contrastive_eval_trials: the single-trial stand-ins, trial by trial, on
    the stacked tensors' slices; NaN where the device call writes nothing."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def clip_train_epoch_trials(self, ti, tt, perm, batch, lr, betas, eps, wd, max_norm, step0, params, m, v,
                                active=None):
        T, N = params.shape[0], ti.shape[0]
        assert 1 <= T <= 16 and params.shape == m.shape == v.shape == (T, 655364) and perm.shape == (T, N)
        active = [True] * T if active is None else list(active)
        self.calls.append(("train", active))
        S = max(-(-N // batch[t]) for t in range(T) if active[t])
        sl, sg = torch.full((T, S), NAN), torch.full((T, S), NAN)
        for t in range(T):
            if active[t]:
                l, n = self.clip_train_epoch(ti, tt, perm[t], batch[t], lr[t], betas, eps, wd[t], max_norm[t], step0[t],
                                             params[t, :R.N_PARAMS], m[t, :R.N_PARAMS], v[t, :R.N_PARAMS])
                sl[t, :len(l)], sg[t, :len(n)] = l, n
        return sl, sg

    def clip_contrastive_eval_trials(self, vi, vt, batch, params, active=None):
        T, N = params.shape[0], vi.shape[0]
        active = [True] * T if active is None else list(active)
        self.calls.append(("eval", active))
        S = max(-(-N // batch[t]) for t in range(T) if active[t])
        bl, cos = torch.full((T, S), NAN), torch.full((T, N), NAN)
        for t in range(T):
            if active[t]:
                l, c = self.clip_contrastive_eval(vi, vt, batch[t], params[t, :R.N_PARAMS])
                bl[t, :len(l)], cos[t] = l, c
        return bl, cos


def _forensics(engine=None, seed=0):
    return types.SimpleNamespace(engine=engine or _TrialsEngine(), clip_state=_clip_state(seed), vault_loaded=False)


# ---- sample_trials ----
def test_sample_trials_is_seeded_and_stays_inside_the_search_space():
    a, b, c = CT.sample_trials(200, 3), CT.sample_trials(200, 3), CT.sample_trials(200, 4)
    assert a == b and a != c and len(a) == 200
    assert CT.sample_trials(5, 3) == a[:5]  # a longer study extends a shorter one
    for t in a:
        assert set(t) == {"lr", "batch_size", "epochs"}
        assert isinstance(t["lr"], float) and 1e-5 <= t["lr"] <= 1e-3
        assert isinstance(t["batch_size"], int) and t["batch_size"] in (8, 12, 16)
        assert isinstance(t["epochs"], int) and 5 <= t["epochs"] <= 15
    assert {t["batch_size"] for t in a} == {8, 12, 16} and {t["epochs"] for t in a} == set(range(5, 16))
    logs = np.log10([t["lr"] for t in a])  # log-uniform: each decade gets its share
    assert 60 < (logs < -4).sum() < 140
    assert CT.sample_trials(0, 1) == []
    assert len(CT.ClipProjectionTuner(_forensics(), n_trials=4, seed=9).trials) == 4
    assert CT.ClipProjectionTuner(_forensics(), n_trials=4, seed=9).trials == CT.sample_trials(4, 9)


# ---- every trial's history is fit's ----
TRIALS = [{"lr": 1e-4, "batch_size": 8, "epochs": 3}, {"lr": 5e-4, "batch_size": 16, "epochs": 1},
          {"lr": 3e-5, "batch_size": 12, "epochs": 2, "seed": 11, "weight_decay": 0.0},
          {"lr": 1e-4, "batch_size": 8, "epochs": 3}]


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    """(result, forensics after tune, checkpoint path, the data, per trial what fit gives alone: history and the
    forensics it left)."""
    ti, tt = R.draws(20, 2)
    vi, vt = R.draws(10, 3)
    labels = np.arange(10) % 2
    alone = []
    for t in TRIALS:
        f = _forensics()
        hist = CT.ClipProjectionTrainer(f, batch_size=t["batch_size"], epochs=t["epochs"], lr=t["lr"],
                                        weight_decay=t.get("weight_decay", 0.01), seed=t.get("seed", 5)).fit(
            (ti, tt), (vi, vt), labels)
        alone.append((hist, f))
    f = _forensics()
    path = str(tmp_path_factory.mktemp("tune") / "clip_detective_best.pth")
    res = CT.ClipProjectionTuner(f, trials=copy.deepcopy(TRIALS), seed=5).tune((ti, tt), (vi, vt), labels,
                                                                              checkpoint_path=path)
    return res, f, path, (ti, tt, vi, vt, labels), alone


def _value(hist):
    best = max(hist, key=lambda h: (h["val_accuracy"], -h["epoch"]))  # the first epoch reaching the best accuracy
    return (best["val_loss"] if best["val_accuracy"] > 0 else float("inf")), best


def test_every_trial_has_the_history_fit_gives_it_alone(study):
    res, f, _, _, alone = study
    assert set(res) == {"best_trial", "best_value", "best_params", "trials"}
    assert [t["number"] for t in res["trials"]] == [0, 1, 2, 3]
    for t, want, (hist, _) in zip(res["trials"], TRIALS, alone):
        assert set(t) == {"number", "params", "value", "history"}
        assert t["params"] == {k: want[k] for k in ("lr", "batch_size", "epochs")}
        assert len(hist) == want["epochs"] and t["history"] == hist  # value for value
        assert t["value"] == _value(hist)[0]
    # epoch e runs the trials with epochs > e: one training and one validation call each
    assert f.engine.calls == [(kind, act) for act in ([True] * 4, [True, False, True, True], [True, False, False, True])
                              for kind in ("train", "eval")]


def test_the_study_minimises_the_loss_at_the_best_accuracy_epoch(study):
    res, f, _, _, alone = study
    values = [_value(h)[0] for h, _ in alone]
    assert values[0] == values[3]  # the same trial twice
    want = min(range(4), key=lambda i: (values[i], i))
    assert res["best_trial"] == want and res["best_value"] == values[want]
    assert res["best_params"] == res["trials"][want]["params"]
    # the winner's best-epoch heads are installed: what fit alone installed for that trial
    assert np.array_equal(CT.flatten_heads(f.clip_state).numpy(), CT.flatten_heads(alone[want][1].clip_state).numpy())
    assert len(f.engine.projections) == 1


class _ScriptedEngine(_TrialsEngine):
    """Validation results by script: (accuracy, loss) per trial and epoch, one validation batch of 8 rows with
    labels 1 1 1 1 0 0 0 0 (the lower median of 0..7 is 3: cosines <= 3 predict 1)."""
    COS = {1.0: [0, 1, 2, 3, 4, 5, 6, 7], 0.5: [0, 1, 6, 7, 2, 3, 4, 5], 0.0: [4, 5, 6, 7, 0, 1, 2, 3]}
    LABELS = np.array([1, 1, 1, 1, 0, 0, 0, 0])

    def __init__(self, script, nan_train=()):
        super().__init__()
        self.script, self.nan_train, self.epoch = script, set(nan_train), 0

    def clip_train_epoch_trials(self, *a, active=None, **k):
        sl, sg = super().clip_train_epoch_trials(*a, active=active, **k)
        for t, e in self.nan_train:
            if e == self.epoch:
                sl[t, 0] = NAN
        return sl, sg

    def clip_contrastive_eval_trials(self, vi, vt, batch, params, active=None):
        T = params.shape[0]
        bl, cos = torch.full((T, 1), NAN), torch.full((T, 8), NAN)
        for t in range(T):
            if active[t]:
                acc, loss = self.script[t][self.epoch]
                bl[t, 0], cos[t] = loss, torch.tensor(self.COS[acc], dtype=torch.float32)
        self.calls.append(("eval", list(active)))
        self.epoch += 1
        return bl, cos


def _scripted(script, nan_train=(), tmp_path=None):
    eng = _ScriptedEngine(script, nan_train)
    f = _forensics(eng)
    ti, tt = R.draws(8, 2)
    trials = [{"lr": 1e-4, "batch_size": 8, "epochs": len(s)} for s in script]
    res = CT.ClipProjectionTuner(f, trials=trials).tune((ti, tt), (ti, tt), eng.LABELS,
                                                        checkpoint_path=tmp_path and str(tmp_path / "ck.pth"))
    return res, f


def test_best_trial_rule_with_a_tie():
    script = [[(0.5, 2.0), (1.0, 1.5), (1.0, 0.125)],  # the FIRST epoch at the best accuracy counts: 1.5
              [(0.5, 0.0625), (1.0, 1.25), (0.5, 0.25)],  # 1.25, not its lowest loss
              [(1.0, 1.25)],                          # a tie with trial 1: the lower number wins
              [(0.0, 0.015625), (0.0, 0.015625)]]     # never better than accuracy 0: inf, as the reference's objective
    res, _ = _scripted(script)
    assert [t["value"] for t in res["trials"]] == [1.5, 1.25, 1.25, float("inf")]
    assert res["best_trial"] == 1 and res["best_value"] == 1.25
    assert [[(h["val_accuracy"], h["val_loss"]) for h in t["history"]] for t in res["trials"]] == script
    res, _ = _scripted([script[2], script[1], script[0]])
    assert res["best_trial"] == 0


def test_a_non_finite_trial_gets_inf_and_the_study_goes_on(tmp_path):
    script = [[(1.0, 0.5), (1.0, 0.25), (1.0, 0.25)],  # its training loss turns NaN in epoch 1
              [(0.5, 1.0), (1.0, 0.75), (0.5, 0.5)],
              [(1.0, NAN), (1.0, 0.125)]]              # a NaN validation loss in epoch 0
    res, f = _scripted(script, nan_train=[(0, 1)], tmp_path=tmp_path)
    assert [t["value"] for t in res["trials"]] == [float("inf"), 0.75, float("inf")]
    assert res["best_trial"] == 1 and res["best_value"] == 0.75
    assert [len(t["history"]) for t in res["trials"]] == [1, 3, 0]  # the entries before the failure stay
    # a failed trial trains no further
    assert [a for k, a in f.engine.calls if k == "train"] == [[True] * 3, [True, True, False], [False, True, False]]
    assert torch.load(str(tmp_path / "ck.pth"), weights_only=True)["epoch"] == 1
    # every trial failed: nothing is installed or written
    res, f = _scripted([[(1.0, NAN)], [(0.0, 0.5)]], tmp_path=tmp_path / "none")
    assert res["best_trial"] == 0 and res["best_value"] == float("inf") and f.engine.projections == []


def test_the_winners_checkpoint_round_trips(study):
    import mmf_amd.vault_builder as VB
    res, f, path, (ti, tt, vi, vt, labels), alone = study
    win = res["best_trial"]
    t = TRIALS[win]
    value, best = _value(alone[win][0])
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "val_loss",
                       "val_accuracy", "train_loss"}
    assert ck["epoch"] == best["epoch"] and ck["val_loss"] == value == res["best_value"]
    assert ck["val_accuracy"] == best["val_accuracy"] and ck["train_loss"] == best["train_loss"]
    sd, meta = VB.load_clip_detective_checkpoint(path)
    assert set(sd) == set(f.clip_state) and meta == {"epoch": best["epoch"], "val_accuracy": best["val_accuracy"]}
    assert np.array_equal(CT.flatten_heads(sd).numpy(), CT.flatten_heads(f.clip_state).numpy())
    # the moments and the step count are that trial's at that epoch: the restatement, run alone
    p = CT.flatten_heads(_clip_state()).numpy().copy()
    m, v, step0 = np.zeros_like(p), np.zeros_like(p), 0
    for perm, lr in CT.plan(20, t["epochs"], t["lr"], t.get("seed", 5))[:best["epoch"] + 1]:
        ls, _, _, _ = R.epoch(ti, tt, perm, t["batch_size"], lr, step0, p, m, v, np.float32,
                              wd=t.get("weight_decay", 0.01))
        step0 += len(ls)
    assert np.array_equal(CT.flatten_heads(sd).numpy(), p)
    det = _Detective()
    opt = torch.optim.AdamW([q for q in det.parameters() if q.requires_grad], lr=t["lr"], weight_decay=0.5)
    opt.load_state_dict(ck["optimizer_state_dict"])
    for q, sl in ((det.clip.visual_projection.weight, slice(0, R.NV)),
                  (det.clip.text_projection.weight, slice(R.NV, R.NV + R.NT)),
                  (det.clip.logit_scale, slice(R.NV + R.NT, None))):
        st = opt.state[q]
        assert float(st["step"]) == step0 and st["exp_avg"].shape == q.shape
        assert np.array_equal(st["exp_avg"].reshape(-1).numpy(), m[sl])
        assert np.array_equal(st["exp_avg_sq"].reshape(-1).numpy(), v[sl])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=t["epochs"], eta_min=t["lr"] * 0.01)
    sched.load_state_dict(ck["scheduler_state_dict"])
    assert sched.last_epoch == ck["epoch"] + 1 and opt.param_groups[0]["lr"] == sched.get_last_lr()[0]
    assert opt.param_groups[0]["weight_decay"] == t.get("weight_decay", 0.01)


def test_more_than_sixteen_trials_run_in_groups():
    eng = _TrialsEngine()
    f = _forensics(eng)
    ti, tt = R.draws(4, 2)
    trials = [{"lr": 1e-4 * (1 + i), "batch_size": 4, "epochs": 1} for i in range(18)]
    res = CT.ClipProjectionTuner(f, trials=trials).tune((ti, tt), (ti, tt), [1, 1, 0, 0])
    assert [len(a) for k, a in eng.calls] == [16, 16, 2, 2] and len(res["trials"]) == 18
    assert res["trials"][17]["params"]["lr"] == trials[17]["lr"] and len(res["trials"][17]["history"]) == 1
    for bad in ([], [{"lr": 1e-4, "batch_size": 65, "epochs": 1}], [{"lr": 1e-4, "batch_size": 8, "epochs": 0}],
                [{"lr": 0.0, "batch_size": 8, "epochs": 1}]):
        with pytest.raises(ValueError):
            CT.ClipProjectionTuner(f, trials=bad)


# ---- the command line ----
def test_tune_flag_runs_the_study_from_two_csvs(tmp_path, capsys, monkeypatch):
    import pandas as pd
    from PIL import Image
    import mmf_amd.api
    paths = _images(tmp_path, 9, Image)
    tr_csv, va_csv = str(tmp_path / "clip_train.csv"), str(tmp_path / "clip_val.csv")
    pd.DataFrame({"text": [f"caption {'w ' * i}" for i in range(9)], "image_path": paths,
                  "label": [0, 0, 1, 0, 0, 1, 0, 0, 0]}).to_csv(tr_csv, index=False)
    pd.DataFrame({"text": [f"other {'v ' * i}" for i in range(5)], "image_path": paths[:5],
                  "label": [0, 1, 0, 1, 1]}).to_csv(va_csv, index=False)
    f = _StubForensics(max_batch=4)
    f.engine.__class__ = _TrialsEngine
    f.engine.calls = []
    monkeypatch.setattr(mmf_amd.api, "MisinfoForensics", lambda device="cuda": f)
    tuned = []
    tune = CT.ClipProjectionTuner.tune

    def spy(self, *a, **k):
        tuned.append((self, tune(self, *a, **k)))
        return tuned[-1][1]
    monkeypatch.setattr(CT.ClipProjectionTuner, "tune", spy)
    ck = str(tmp_path / "out.pth")
    CT.main(["--tune", "--trials", "3", "--train-csv", tr_csv, "--val-csv", va_csv, "--checkpoint", ck])
    out = capsys.readouterr().out
    assert "Number of trials: 3" in out and "Filtered to 7 matched pairs (from 9 total)" in out
    (tuner, res), = tuned
    assert tuner.trials == CT.sample_trials(3, 0) and len(res["trials"]) == 3
    assert f.chunks == [4, 3, 4, 1]  # ONE feature extraction for the whole study
    assert f"Best trial: {res['best_trial']}" in out and f"Best val loss: {res['best_value']:.4f}" in out
    for k, v in res["best_params"].items():
        assert f"  {k}: {v}" in out
    assert [len(t["history"]) for t in res["trials"]] == [t["epochs"] for t in tuner.trials]
    # without --tune the command trains once, as before
    CT.main(["--train-csv", tr_csv, "--val-csv", va_csv, "--epochs", "1", "--batch-size", "4", "--checkpoint", ck])
    assert len(tuned) == 1 and "Epoch 1/1" in capsys.readouterr().out
    assert CT.run_hyperparameter_tuning(2, str(tmp_path / "none.csv"), va_csv) is None
