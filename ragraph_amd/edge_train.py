"""Staged fine-tuning of the link-prediction flavour: the reference's RAGraph_edge/finetune_rag.py:55-171 driver and its
utils/trainer.py Trainer, on ragraph_amd.

    for stage s = 1 .. len(test_files):                        files = [pretrain, fine_tune, test_1, ..., test_n]
        state  = the pre-trained tables, or -- once updt_inter stages are saved -- their interpolative update with the
                 last updt_inter saved models, row-normalised                        finetune_rag.py:63-94
        prompt = EdgeListData(merge_frames(files[:s + 1]), sizes of the pre-training dataset)          :106-138
        pre    = RAGraph(prompt, phase="for_tune"), state loaded strictly, eval mode                   :141-145
        data   = EdgeListData(files[s], test_s, phase="finetune", user_hist_files=files[:s])           :147-154
        model  = RAGraph(data, pre, phase="finetune")                                                  :155
        Trainer(data).train_finetune(model, pre)                                                       :157-163

The interpolative update is one kernel call per table (kernels.interp_normalize: the tables read once, one written), where
the reference stacks the S tables, multiplies, sums and normalises (4S + 4 passes and two [S, n, D] temporaries)."""
from __future__ import annotations

import datetime
import itertools
import os
import time

import numpy as np
import torch
import torch.nn.functional as F

from . import kernels as K
from ._native import INTERP_MAX_TABLES
from .edge_data import EdgeListData, merge_frames, read_frame
from .edge_eval import Metric
from .RAGraph_edge import RAGraph

TABLE_PREFIXES = ("user_embedding", "item_embedding")   # finetune_rag.py:82,93
MODEL_ATTRS = ("dropout_rng", "noise_rng", "loss_rows")   # model_kwargs that are attributes of RAGraph, not constructor arguments
_save_counter = itertools.count()


class Trainer:
    """utils/trainer.py:10-133, the reference's arguments (--lr, --batch_size, --num_epochs, --early_stop_patience,
    --save_dir) as constructor parameters.  save_dir=None keeps the best state dict in memory (`best_state`: cloned device
    tensors) where the reference writes a file; otherwise it is written with torch.save and `save_path` names it.
    log: a callable taking one string, or None."""

    def __init__(self, dataset, pre_dataset=None, metric=None, lr=1e-3, batch_size=2048, num_epochs=300,
                 early_stop_patience=10, save_dir=None, log=None):
        self.dataloader = dataset
        self.pre_dataloader = pre_dataset
        self.metric = metric if metric is not None else Metric("recall;ndcg", "20", 512)
        self.lr, self.batch_size, self.num_epochs = lr, int(batch_size), int(num_epochs)
        self.early_stop_patience = int(early_stop_patience)
        self.save_dir, self._log = save_dir, log
        self.best_perform = {'recall': [0.], 'ndcg': [0.]}
        self.best_state = self.save_path = None
        self.stop_counter, self.stop_flag = 0, False
        self._exp_time = datetime.datetime.now().strftime("%b-%d-%Y_%H-%M-%S") + f"_{next(_save_counter)}"

    def log(self, msg):
        if self._log is not None:
            self._log(msg)

    def create_optimizer(self, model):
        self.optimizer = torch.optim.Adam(model.parameters(), lr=self.lr)    # trainer.py:18-21

    def train_epoch(self, model, epoch_idx):
        """trainer.py:23-59: shuffle, then whole batches only (the tail is dropped); the logged loss terms are divided by
        num_edges // batch_size + 1, as the reference divides them."""
        data, bs = self.dataloader, self.batch_size
        data.shuffle()
        s, loss_log_dict = 0, {}
        t0 = time.time()
        model.train()
        while s + bs <= data.num_edges:
            batch_data = data.get_train_batch(s, s + bs)
            self.optimizer.zero_grad()
            loss, loss_dict = model.cal_loss(batch_data)
            loss.backward()
            self.optimizer.step()
            for name in loss_dict:
                val = float(loss_dict[name]) / (data.num_edges // bs + 1)
                loss_log_dict[name] = loss_log_dict.get(name, 0.0) + val
            s += bs
            if self.stop_flag:
                break
        loss_log_dict['train_time'] = round(time.time() - t0, 2)
        self.log(f"epoch {epoch_idx}: " + " ".join(f"{k} {v:.6g}" for k, v in loss_log_dict.items()))
        return loss_log_dict

    def _loop(self, model):
        self.create_optimizer(model)
        self.best_perform = {'recall': [0.], 'ndcg': [0.]}
        self.stop_counter, self.stop_flag = 0, False
        for epoch_idx in range(self.num_epochs):
            self.train_epoch(model, epoch_idx)
            self.evaluate(model, epoch_idx, self.dataloader)
            if self.stop_flag:
                break
        return self.best_perform

    def train(self, model):
        """trainer.py:62-75."""
        return self._loop(model)

    def train_finetune(self, model, pre_model):
        """trainer.py:78-99."""
        pre_model.eval()
        return self._loop(model)

    def evaluate(self, model, epoch_idx, dataloader):
        """trainer.py:101-122: only a recall[0] STRICTLY above the best so far counts, saves the model and resets the
        counter; `early_stop_patience` evaluations in a row without one set stop_flag."""
        model.eval()
        eval_result = self.metric.eval(model, dataloader)
        self._log_eval(eval_result)
        if eval_result['recall'][0] > self.best_perform['recall'][0]:
            self.best_perform = eval_result
            self.log(f"Find better model at epoch: {epoch_idx}: recall={self.best_perform['recall'][0]}")
            self.save_model(model)
            self.stop_counter = 0
        else:
            self.stop_counter += 1
            if self.stop_counter >= self.early_stop_patience:
                self.log(f"Early stop! Best performance: recall={self.best_perform['recall'][0]}, "
                         f"ndcg={self.best_perform['ndcg'][0]}")
                self.stop_flag = True
        model.train()

    def test(self, model, dataloader):
        """trainer.py:124-129."""
        model.eval()
        eval_result = self.metric.eval(model, dataloader)
        self._log_eval(eval_result)
        return eval_result

    def _log_eval(self, eval_result):
        if self._log is not None:
            self.log(" ".join(f"{m}@{self.metric.k}: {np.asarray(eval_result[m]).tolist()}" for m in eval_result
                              if m != "eval_time"))

    def save_model(self, model):
        """trainer.py:131-133."""
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        if self.save_dir is None:
            self.best_state = state
        else:
            os.makedirs(self.save_dir, exist_ok=True)
            self.save_path = os.path.join(self.save_dir, f"saved_model_{self._exp_time}.pt")
            torch.save(state, self.save_path)


def interpolation_weights(interval, pretrain_weight=0.5):
    """finetune_rag.py:70-79, computed as written there (torch fp32 on the CPU): [p, (1 - p) * normalize_1(1..I).flip()],
    the weights of [pre-trained, newest saved, ..., oldest of the I]."""
    interpolative_weight = (1 - pretrain_weight) * F.normalize(
        torch.arange(1, interval + 1).float(), dim=0, p=1
    ).flip(dims=[0])
    return torch.cat([torch.tensor([pretrain_weight]), interpolative_weight])


def interpolative_update(pre_state, saved_states, pretrain_weight=0.5, device="cuda"):
    """finetune_rag.py:64-86: for every user_embedding* / item_embedding* key of the PRE-TRAINING state dict, the
    row-normalised mix of [pre, saved[-1], saved[-2], ...] under interpolation_weights(len(saved_states)).  No other key
    enters: a fine-tuned model's gate and LoRA factors are not keys of the pre-training checkpoint."""
    saved_states = list(saved_states)
    if not 1 <= len(saved_states) <= INTERP_MAX_TABLES - 1:
        raise ValueError(f"interpolative_update: {len(saved_states)} saved states, not 1 to {INTERP_MAX_TABLES - 1}")
    weights = interpolation_weights(len(saved_states), pretrain_weight)
    states = [pre_state] + saved_states[::-1]
    return {k: K.interp_normalize([sd[k].detach().to(device=device, dtype=torch.float32) for sd in states], weights)
            for k in pre_state if k.startswith(TABLE_PREFIXES)}


def run_stages(pretrain_file, pretrain_val_file, finetune_file, test_files, pre_state, updt_inter=1, model_kwargs=None,
               trainer_kwargs=None, hour_interval_pre=1, hour_interval_f=1, device="cuda", on_stage=None):
    """finetune_rag.py:55-171.  pre_state: the pre-training state dict (the reference's --pre_model_path, loaded).
    model_kwargs: RAGraph's constructor arguments for the fine-tuned model (emb_size and num_layers also go to the for_tune
    model), and the attributes MODEL_ATTRS (e.g. dropout_rng="device"), which are set on it.
    on_stage(stage, pre_model, model, trainer), if given, is called after every stage's training.
    Returns {"recalls", "ndcgs": per stage; "recall_mean", "recall_std", "ndcg_mean", "ndcg_std": rounded to 5 places as
    the reference logs them; "states": the best state dict of every stage}.  A stage whose model never beat recall 0 has
    saved nothing (the reference dies there on trainer.save_path): RuntimeError."""
    if not 1 <= updt_inter <= INTERP_MAX_TABLES - 1:
        raise ValueError(f"updt_inter={updt_inter}: 1 to {INTERP_MAX_TABLES - 1}")
    model_kwargs, trainer_kwargs = dict(model_kwargs or {}), dict(trainer_kwargs or {})
    model_attrs = {k: model_kwargs.pop(k) for k in MODEL_ATTRS if k in model_kwargs}
    all_data = [pretrain_file, finetune_file, *test_files]
    pretrain_dataset = EdgeListData(pretrain_file, pretrain_val_file, hour_interval=hour_interval_pre, device=device)
    all_frames = [read_frame(f) for f in all_data]
    saved_states, recalls, ndcgs = [], [], []
    for num_stage in range(1, len(test_files) + 1):
        if len(saved_states) >= updt_inter:
            state_dict = interpolative_update(pre_state, saved_states[-updt_inter:], device=device)
        else:
            state_dict = pre_state
        new_state_dict = {k: v for k, v in state_dict.items() if k.startswith(TABLE_PREFIXES)}
        test_data_idx = num_stage + 1
        ft_data_idx = test_data_idx - 1
        # structural prompt: propagate over everything seen so far, in the pre-training dataset's id space
        pre_dataset = EdgeListData(merge_frames(all_frames[:ft_data_idx + 1]), all_frames[ft_data_idx], has_time=True,
                                   hour_interval=hour_interval_pre, pre_dataset=pretrain_dataset, device=device)
        pretrained_model = RAGraph(pre_dataset, None, phase="for_tune", device=device,
                                   **{k: model_kwargs[k] for k in ("emb_size", "num_layers") if k in model_kwargs})
        pretrained_model.load_state_dict(new_state_dict, strict=True)
        pretrained_model.eval()
        finetune_dataset = EdgeListData(all_data[ft_data_idx], test_files[num_stage - 1], phase="finetune",
                                        pre_dataset=pre_dataset, has_time=True, user_hist_files=all_data[:ft_data_idx],
                                        hour_interval=hour_interval_f, device=device)
        model = RAGraph(finetune_dataset, pretrained_model, phase="finetune", device=device, **model_kwargs)
        for k, v in model_attrs.items():
            setattr(model, k, v)
        trainer = Trainer(finetune_dataset, pre_dataset=pretrain_dataset, **trainer_kwargs)
        best_perform = trainer.train_finetune(model, pretrained_model)
        if on_stage is not None:
            on_stage(num_stage, pretrained_model, model, trainer)
        if trainer.best_state is None and trainer.save_path is None:
            raise RuntimeError(f"stage {num_stage}: the model never improved on recall 0, so there is no saved model "
                               "for the next stage to start from")
        recalls.append(best_perform["recall"][0])
        ndcgs.append(best_perform["ndcg"][0])
        saved_states.append(trainer.best_state if trainer.best_state is not None
                            else torch.load(trainer.save_path, map_location=device))
    return {"recalls": recalls, "ndcgs": ndcgs,
            "recall_mean": np.round(np.mean(recalls), 5), "recall_std": np.round(np.std(recalls), 5),
            "ndcg_mean": np.round(np.mean(ndcgs), 5), "ndcg_std": np.round(np.std(ndcgs), 5), "states": saved_states}
