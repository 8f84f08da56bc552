"""Eager against captured (ragraph_amd.capture.CapturedTrainStep) fine-tuning steps, in one process, alternating.

    python tools/capture_train_probe.py [--steps 200] [--rounds 4] [--only node_528|fewshot]

Shapes: `node_528` is tools/bench_blocks.py finetune_node("528") (16 ENZYMES-style graphs, ~530 nodes, 20 000 x 256 bank,
k = 4, decoder head trained); `fewshot` is the node few-shot step of RAGraph_node_fewshot/finetune-rag.py:94-103 (8 graphs,
support-set inference, prototype means, retrieval with position codes, decode layer + PReLU slope trained, prototype
cosine, cross entropy).  Every variant runs `steps` steps per round, the variants take turns for `rounds` rounds, and the
median round is reported (ms per step, CUDA events around the whole block, host time included):
    eager        the eager step with the same capturable Adam the graph runs
    eager_foreach  (node_528) the eager step with torch's default Adam -- what bench.py times
    eager_host_slope (fewshot) the eager step as it ran before the device-slope entries: the trained layer's slope read
                 on the host in its training branch AND in the support-set inference's epilogue (one read-back per
                 step, after each Adam update)
    replay       the captured step
One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def node_528(dev, capturable=True):
    from ragraph_amd.data import DataLoader, synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph import RAGraph
    from ragraph_amd.ragraph_utils import process_tu_dataset

    F_in, C, D, N = 18, 3, 256, 20_000
    ds = synthetic_tu_dataset(num_graphs=16, num_node_attributes=F_in, num_node_labels=C, seed=21)
    feats, adj, _ = process_tu_dataset(next(iter(DataLoader(ds, batch_size=16))), F_in, device=dev)
    _ = adj.row_normalized_values()
    gen = torch.Generator(device=dev).manual_seed(74)
    torch.manual_seed(5)
    model = RAGraph(PrePrompt(F_in, D, "prelu", 1, 0.3).to(dev), None, F_in, C, D, finetune=True, device=dev)
    model.toy_graph_base.add_resources(F.normalize(torch.randn(N, D, device=dev, generator=gen), dim=-1),
                                       torch.randn(N, D, device=dev, generator=gen),
                                       F.one_hot(torch.randint(0, C, (N,), device=dev, generator=gen), C).float())
    labels = torch.randint(0, C, (feats.shape[0],), device=dev, generator=torch.Generator(device=dev).manual_seed(75))
    model.train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3, capturable=capturable)
    return model, (lambda x, y: F.cross_entropy(model(x, adj), y)), opt, (feats, labels)


def fewshot(dev):
    from ragraph_amd.data import DataLoader, synthetic_tu_dataset
    from ragraph_amd.preprompt import PrePrompt
    from ragraph_amd.RAGraph_fewshot import RAGraph as RAGraphFewShot
    from ragraph_amd.ragraph_utils import fewshot_mean_logits, fewshot_predict_logits, process_tu_dataset

    F_in, C, D = 18, 3, 256
    ds = synthetic_tu_dataset(num_graphs=8, num_node_attributes=F_in, num_node_labels=C, seed=8)
    feats, adj, node_oh = process_tu_dataset(next(iter(DataLoader(ds, batch_size=8))), F_in, device=dev)
    sup = synthetic_tu_dataset(num_graphs=2, num_node_attributes=F_in, num_node_labels=C, seed=9)
    sfeat, sadj, _ = process_tu_dataset(next(iter(DataLoader(sup, batch_size=2))), F_in, device=dev)
    slabels = torch.arange(sfeat.shape[0], device=dev) % C
    _ = adj.row_normalized_values(), sadj.row_normalized_values()
    gen = torch.Generator(device=dev).manual_seed(4)
    torch.manual_seed(12)
    pre = PrePrompt(F_in, D, "prelu", 2, 0.3).to(dev)
    model = RAGraphFewShot(pre, None, torch.zeros(C, D, device=dev), D, device=dev, dataset_name="ENZYMES")
    model.toy_graph_base.add_resources(F.normalize(torch.randn(600, D, device=dev, generator=gen), dim=-1),
                                       torch.randn(600, D, device=dev, generator=gen),
                                       F.one_hot(torch.randint(0, C, (600,), device=dev, generator=gen), C).float(),
                                       torch.rand(600, 10, device=dev, generator=gen))
    anchors = torch.randint(0, feats.shape[0], (10,), device=dev, generator=gen)
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)

    def step(x, y):
        mean = fewshot_mean_logits(pre.inference(sfeat, sadj), slabels, num_class=C)
        return F.cross_entropy(fewshot_predict_logits(mean, model(x, adj, mean, anchors=anchors)), y)
    return model, step, opt, (feats, node_oh.argmax(dim=1))


class host_slope:
    """The trained GCN layer's training branch as it was before the device-slope entries: slope read on the host."""

    def __enter__(self):
        from ragraph_amd import autograd as A
        from ragraph_amd import kernels as K
        from ragraph_amd.layers import gcn

        self.orig = gcn.GCN.forward

        def forward(layer, input, sparse=False):
            x = input[0].squeeze(0) if input[0].dim() == 3 else input[0]
            if torch.is_grad_enabled() and any(p.requires_grad for p in layer.parameters()):
                g = gcn.as_csr(input[1])
                return A.spmm_csr(g, A.linear(x, layer.fc.weight), layer.bias, K.ACT_PRELU, layer.act.weight,
                                  layer._alpha())
            if gcn.sparse_features(x, probe=False) is None and not gcn.aggregate_first(x.shape[1], layer.fc.weight.shape[0]):
                # the plain inference epilogue with the host slope too (the support-set inference of the few-shot step)
                g = gcn.as_csr(input[1])
                return K.spmm_csr(g.rowptr, g.col, g.val, K.linear(x, layer.fc.weight), bias=layer.bias, act=K.ACT_PRELU,
                                  alpha=layer._alpha(), long_rows=g.has_long_rows)
            return self.orig(layer, input, sparse)
        gcn.GCN.forward = forward

    def __exit__(self, *a):
        from ragraph_amd.layers import gcn
        gcn.GCN.forward = self.orig


def eager_loop(step, opt, inputs, steps):
    def run():
        for _ in range(steps):
            opt.zero_grad()
            step(*inputs).backward()
            opt.step()
    return run


def time_block(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--only", default=None)
    ap.add_argument("--variants", default=None, help="comma-separated subset of the variants (a profiler run of one)")
    args = ap.parse_args()
    from ragraph_amd.capture import CapturedTrainStep

    dev = torch.device("cuda:0")
    for shape in ("node_528", "fewshot"):
        if args.only and shape != args.only:
            continue
        make = node_528 if shape == "node_528" else fewshot
        variants = {}
        _, step_e, opt_e, ins = make(dev)
        variants["eager"] = eager_loop(step_e, opt_e, ins, args.steps)
        if shape == "node_528":
            _, step_f, opt_f, _ = node_528(dev, capturable=False)
            variants["eager_foreach"] = eager_loop(step_f, opt_f, ins, args.steps)
        else:
            _, step_h, opt_h, _ = make(dev)
            loop_h = eager_loop(step_h, opt_h, ins, args.steps)

            def with_host_slope():
                with host_slope():
                    loop_h()
            variants["eager_host_slope"] = with_host_slope
        _, step_c, opt_c, _ = make(dev)
        cap = CapturedTrainStep(step_c, opt_c, *ins)

        def replay():
            for _ in range(args.steps):
                cap(*ins)
        variants["replay"] = replay
        if args.variants:
            variants = {k: v for k, v in variants.items() if k in args.variants.split(",")}
        for fn in variants.values():   # warm every variant once
            fn()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(time_block(fn, args.steps))
        rec = {"shape": shape, "steps_per_round": args.steps, "rounds": args.rounds,
               "ms_per_step": {k: round(statistics.median(v), 4) for k, v in times.items()},
               "all_rounds": {k: [round(x, 4) for x in v] for k, v in times.items()}}
        if "replay" in times and "eager" in times:
            rec["replay_over_eager"] = round(rec["ms_per_step"]["replay"] / rec["ms_per_step"]["eager"], 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
