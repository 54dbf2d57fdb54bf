# coding: utf-8
"""GPU: train.py with gt_mode 'siren' end to end (reference train.py:121-129, :403-447): the signed mesh of every periodic
checkpoint and of the best model when the Lewiner tables are given, and a run that still finishes — losses.csv, model_final.pth,
the field slice — when they are not: the mesh is an optional artefact, a training must not be lost over it."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def siren_config(tmp_path, **extra):
    cfg = json.load(open(os.path.join(os.path.dirname(HERE), "configs", "train_synth_eikonal.json")))
    for k in ("s1_epochs", "warmup_epochs", "loss_s1_weights", "loss_s2_weights"):
        del cfg[k]
    cfg.update({"gt_mode": "siren", "num_epochs": 5, "batch_size": 3000, "resolution": 24, "epochs_to_checkpoint": 2,
                "loss_weights": [3e3, 1e2, 1e2, 5e1], "optimizer": {"type": "adam", "lr": 1e-5},
                "checkpoint_path": str(tmp_path), "experiment_name": "t",
                "network": {"hidden_layer_nodes": [64] * 4, "w0": 30, "pretrained_dict": "None"}})
    cfg.update(extra)
    return cfg


def check_run_finished(base):
    import pandas as pd
    df = pd.read_csv(base / "losses.csv", sep=";")
    assert len(df) == 5 and np.isfinite(df.values).all()
    assert (base / "models" / "model_final.pth").exists() and (base / "models" / "model_best.pth").exists()
    for ep in (2, 4):
        assert (base / "models" / f"model_{ep}.pth").exists(), ep
    assert (base / "reconstructions" / "field_slice.npz").exists()              # generate_df with gt_mode 'siren'


def test_siren_training_writes_its_meshes(tmp_path):
    import train
    from generate_mc import generate_mc
    z = np.load(os.path.join(HERE, "golden", "g10_meshudf.npz"))
    luts = str(tmp_path / "luts.npz")
    np.savez(luts, **{k[4:]: z[k] for k in z.files if k.startswith("lut_")})
    t, mesh = train.setup_train(siren_config(tmp_path, luts_path=luts), 0)
    base = tmp_path / "t"
    check_run_finished(base)
    rec = base / "reconstructions"
    for name in ("mc_mesh_2.obj", "mc_mesh_4.obj", "mc_mesh_best.obj"):
        assert (rec / name).exists() and os.path.getsize(rec / name) > 0, name
    assert not (rec / "mc_mesh_1.obj").exists() and not (rec / "mc_mesh_3.obj").exists()
    assert t > 0 and np.asarray(mesh.faces).shape[1:] == (3,) and len(mesh.faces) > 0
    # the mesh of a periodic checkpoint = the signed mesh of that checkpoint's file
    generate_mc(None, "siren", 0, 24, str(tmp_path / "chk.obj"), algorithm="siren", luts=luts,
                from_file={"w0": 30, "model_path": str(base / "models" / "model_2.pth"), "hidden_layer_nodes": [64] * 4})
    assert open(tmp_path / "chk.obj").read() == open(rec / "mc_mesh_2.obj").read()


def test_siren_training_finishes_without_tables(tmp_path, monkeypatch, capsys):
    import train
    from diffudf_amd import marching_cubes as M
    monkeypatch.delenv("DUDF_MESHUDF_LUTS", raising=False)
    with pytest.raises(M.MeshUDFError):
        M.load_luts(None)                                                       # this environment has no tables to find
    t, mesh = train.setup_train(siren_config(tmp_path), 0)
    check_run_finished(tmp_path / "t")
    assert t > 0 and mesh is None
    rec = tmp_path / "t" / "reconstructions"
    assert not [f for f in os.listdir(rec) if f.startswith("mc_mesh")]
    assert "signed marching cubes skipped" in capsys.readouterr().out
