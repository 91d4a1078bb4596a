#!/usr/bin/env python3
"""The reference's training entry point (train.py:80-504) condensed onto this package's pieces, end to end on synthetic data:

    .npz volumes + CSV  ->  DataPreprocessor (raw volumes from the workers)          gaviko_amd.data          (train.py:33-78)
    batch.to(device)    ->  RandomAffine + RandomFlip + RescaleIntensity on the GPU  gaviko_amd.data          (train.py:38-62)
    build_model(config['model'])                                                     gaviko_amd.registry      (train.py:111-153)
    FocalLoss(gamma=1.2) with device-side running loss / accuracy                    gaviko_amd.losses        (train.py:176-179,327-328)
    clip_grad_norm_(1.0) + Adam + OneCycleLR as one fused step                       gaviko_amd.optim         (train.py:185-206,315-319)
    validation: accuracy / quadratic kappa / macro OvR AUC                           gaviko_amd.metrics       (eval.py:103-122)
    best-model checkpoint with the trainable tensors only                            gaviko_amd.utils         (train.py:460-485)

With --ragged the volumes have shapes and spacings of their own (VolumeDataset + collate_ragged) and data.Conform brings each batch onto
the (120,160,160) grid on the device (Resample to 1 mm, CropOrPad) before the transforms above.

With --histogram the last step is torchio's MRI recipe: data.HistogramStandardization with landmarks trained here on the training volumes, then
ZNormalization above the mean.

usage: python examples/train_synthetic.py [--ragged] [--histogram] [--method gaviko] [--backbone vit-t16] [--epochs 3] [--samples 8] [--out /tmp/gaviko_run]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaviko_amd import data, losses, metrics  # noqa: E402
from gaviko_amd.optim import FusedAdamOneCycle  # noqa: E402
from gaviko_amd.registry import build_model  # noqa: E402
from gaviko_amd.utils import load_pretrained  # noqa: E402


def make_dataset(root, n, num_classes, seed=0, ragged=False):
    """n synthetic (120,160,160) volumes per subset whose class shows in a coarse intensity pattern; CSV with the reference's columns.
    ragged: every volume gets a shape of its own around (130, 170, 170) and a spacing around (0.9, 0.95, 0.95), stored under 'spacing'."""
    import pandas as pd
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(seed)
    rows = []
    for subset, count in (("train", n), ("val", max(num_classes, n // 2)), ("test", max(num_classes, n // 2))):
        for i in range(count):
            k = i % num_classes
            shape = tuple(int(s) for s in rng.integers((110, 150, 150), (150, 190, 190))) if ragged else (120, 160, 160)
            v = rng.standard_normal(shape).astype(np.float32) * 40 + 500
            v[k * shape[0] // 6:(k + 1) * shape[0] // 6] += 400.0        # a bright slab whose depth position is the label
            name = f"{subset}_{i}.npz"
            extra = dict(spacing=np.array([120.0, 160.0, 160.0]) / shape * rng.uniform(0.97, 1.03, 3)) if ragged else {}
            np.savez(os.path.join(root, name), data=v, **extra)
            rows.append(dict(mri_path=name, kl_grade=k, subset=subset))
    csv = os.path.join(root, "data.csv")
    pd.DataFrame(rows).to_csv(csv, index=False)
    return csv


def run(method="gaviko", backbone="vit-t16", epochs=3, samples=8, out="/tmp/gaviko_run", batch_size=4, lr=1e-3, seed=0, log=print, intensity_augment=False,
        motion_augment=False, batch_mix=False, ragged=False, histogram=False, ood_scores=False):
    dev = torch.device("cuda:0")
    K = 5
    csv = make_dataset(os.path.join(out, "data"), samples, K, seed, ragged)
    config = {"data": dict(data_path=csv, image_folder=os.path.join(out, "data"), batch_size=batch_size, num_workers=0,
                           intensity_augment=intensity_augment,          # train.py:43-51: the OneOf(intensity_augment) stage, on the device
                           motion_augment=motion_augment,                # ... with tio.RandomMotion as its fourth member (needs the stage)
                           **({"batch_mix": dict(seed=seed)} if batch_mix else {}),    # Mixup / CutMix of the batch, timm's defaults
                           # raw scans of any shape and spacing: resampled to 1 mm, cropped / padded onto the model's grid, on the device
                           **({"conform": dict(target_shape=(120, 160, 160), spacing=1.0, padding_mode="minimum")} if ragged else {})),
              "model": dict(method=method, backbone=backbone, image_size=160, image_patch_size=16, frames=120, frame_patch_size=12, num_classes=K,
                            channels=1, pool="cls", dim_head=64, dropout=0.1, emb_dropout=0.1, freeze_vit=True, num_prompts=8, prompt_dim=64,
                            prompt_dropout=0.1, deep_prompt=method == "deep_vpt", prompt_latent_dim=20, local_dim=20, local_k=(6, 6, 6),
                            DHW=(10, 10, 10), attn_drop=0.2, proj_drop=0.2, share_factor=1, r=4, alpha=4),
              "train": dict(save_dir=out, save_threshold=0.0)}
    torch.manual_seed(seed)
    pre = data.DataPreprocessor(config, seed=seed)
    train_loader, val_loader, _, train_ds, val_ds, _ = pre.preprocess(None)
    if histogram:       # torchio's recipe: landmarks learned once from the training volumes, then HistogramStandardization + ZNormalization
        on_grid = (lambda batch: pre.conform(batch.to(dev))) if pre.conform is not None else (lambda batch: batch.to(dev))
        path = os.path.join(out, "landmarks.npy")
        landmarks = data.HistogramStandardization.train((on_grid(inputs) for inputs, _ in train_loader), masking_method="mean", output_path=path)
        log(f"histogram landmarks from {len(train_ds)} training volumes: {np.round(landmarks, 2).tolist()}")
        config["data"]["normalization"] = {"histogram": {"landmarks": path, "masking_method": "mean"}, "then": "znorm"}
        pre = data.DataPreprocessor(config, seed=seed)                   # the loaders stay; the transforms now standardise first
    model = build_model(config["model"]).to(dev)
    tuning_params = load_pretrained.tuning_param_names(model)            # train.py:160-169
    log(f"{method}/{backbone}: {len(tuning_params)} trainable tensors, {len(train_ds)} train / {len(val_ds)} val volumes")
    meter = losses.StepMeter(dev)
    criterion = losses.FocalLoss(gamma=1.2).attach_meter(meter)          # train.py:176-177
    total_steps = epochs * len(train_loader)
    opt = FusedAdamOneCycle(model, lr=lr, eps=1e-8, max_norm=1.0, max_lr=lr, total_steps=total_steps, pct_start=0.3, div_factor=10,
                            final_div_factor=1000)
    history, best_acc, best_path = [], -1.0, None
    to_grid = (lambda batch: pre.conform(batch.to(dev, non_blocking=True))) if pre.conform is not None else (lambda batch: batch.to(dev, non_blocking=True))
    for epoch in range(epochs):
        model.train()
        meter.reset()
        for inputs, labels in train_loader:
            inputs, target = pre.train_transforms(to_grid(inputs)), labels.to(dev)
            if pre.batch_mix is not None:                                 # after the normaliser; the target becomes a data.MixedTarget
                inputs, target = pre.batch_mix(inputs, target)
            loss = criterion(model(inputs), target)
            loss.backward()
            opt.step()
            opt.zero_grad()
        train_loss, train_acc, n = meter.read()                         # the epoch's only host read of the training loop
        model.eval()
        ev = metrics.Evaluator(K, dev)
        with torch.no_grad():
            for inputs, labels in val_loader:
                ev.update(model(pre.val_transforms(to_grid(inputs))), labels.to(dev))
        r = ev.compute()
        history.append(dict(epoch=epoch, train_loss=train_loss, train_acc=train_acc, val_acc=r["accuracy"], val_kappa=r["quadratic_kappa"], val_auc=r["auc"]))
        log(f"epoch {epoch}: train loss {train_loss:.4f} acc {train_acc:.3f} | val acc {r['accuracy']:.3f} kappa {r['quadratic_kappa']:.3f} auc {r['auc']}")
        if r["accuracy"] > best_acc:                                      # train.py:460-485
            best_acc = r["accuracy"]
            best_path = load_pretrained.save_trainable(model, out, method, backbone, epoch, best_acc, tuning_params)
    paths = [os.path.join(config["data"]["image_folder"], p) for p in val_ds.df["mri_path"]]
    csv_out = metrics.write_eval_outputs(os.path.join(out, "results"), method, backbone, paths, r["y_pred"], r["accuracy"], r["quadratic_kappa"], r["auc"])
    ood_eval = None
    if ood_scores:      # is a scan the kind of scan the model was trained on?  Gaussians on the training features, then validation volumes
        from gaviko_amd import features, ood                              # against the same volumes behind a strong bias field and ghosting
        embed = lambda x: features.embed(model, pre.val_transforms(x)).pooled      # noqa: E731
        feats, labs = zip(*[(embed(to_grid(inputs)), labels.to(dev)) for inputs, labels in train_loader])
        fit = ood.fit_gaussian(torch.cat(feats), torch.cat(labs), K)
        shift = data.DeviceCompose([data.RandomBiasField(coefficients=1.0), data.RandomGhosting(num_ghosts=(6, 10), intensity=(1.0, 2.0))], seed=seed)
        s_in, s_out = [], []
        for inputs, _ in val_loader:
            x = to_grid(inputs)
            s_in.append(fit.relative(embed(x.clone()))[0])
            s_out.append(fit.relative(embed(shift(x.clone())))[0])
        ood_eval = ood.evaluate(torch.cat(s_in), torch.cat(s_out), replicates=200, seed=seed)
        log(f"ood (relative Mahalanobis, shrinkage {fit.shrinkage:.3f} / {fit.shrinkage0:.3f}): val vs bias field + ghosting: auroc {ood_eval.auroc:.3f} "
            f"{tuple(round(v, 3) for v in ood_eval.auroc_ci)} fpr95 {ood_eval.fpr95:.3f} aupr {ood_eval.aupr:.3f}")
    return dict(history=history, checkpoint=best_path, results_csv=csv_out, model=model, config=config, pre=pre, val_loader=val_loader, ood=ood_eval)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", default="gaviko")
    ap.add_argument("--backbone", default="vit-t16")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--out", default="/tmp/gaviko_run")
    ap.add_argument("--intensity-augment", action="store_true", help="add noise / bias field / blur (one of, p=0.75) to the train transforms")
    ap.add_argument("--motion-augment", action="store_true", help="with --intensity-augment: add k-space motion as the fourth member of that group")
    ap.add_argument("--batch-mix", action="store_true", help="Mixup / CutMix of each training batch (data.BatchMix, timm's defaults) with the mixed-target loss")
    ap.add_argument("--ragged", action="store_true", help="synthetic volumes of unequal shape and spacing, brought onto the grid by data.Conform")
    ap.add_argument("--histogram", action="store_true", help="train histogram landmarks on the synthetic training volumes (on the device) and "
                    "normalise with data.HistogramStandardization followed by ZNormalization instead of the min-max rescale")
    ap.add_argument("--ood", action="store_true", help="after training: fit ood.fit_gaussian on the training features and score the validation volumes "
                    "against the same volumes behind a strong RandomBiasField + RandomGhosting (ood.evaluate)")
    a = ap.parse_args()
    res = run(a.method, a.backbone, a.epochs, a.samples, a.out, intensity_augment=a.intensity_augment, motion_augment=a.motion_augment,
              batch_mix=a.batch_mix, ragged=a.ragged, histogram=a.histogram, ood_scores=a.ood)
    print("checkpoint:", res["checkpoint"])
    print("results   :", res["results_csv"])
