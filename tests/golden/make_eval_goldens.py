#!/usr/bin/env python3
"""Generate the evaluation-engine fixture by RUNNING THE REAL REFERENCE (build container only):

  eval_engine.json   engine/engine_for_slot.py final_test_with_scene_label on stub modules that replay seeded tensors (CPU), and merge on seeded
                     prediction files: the inputs, the exact text of every file written / read, the returned values

The reference's engine imports timm.utils.accuracy; timm is not in the build container, so timm 0.4.12's accuracy (eight lines) is restated here and
handed to the reference as that module's function, the way make_goldens.install_reference() hands it timm's drop_path.  The fixture is data only.

Usage (in the build container):  python tests/golden/make_eval_goldens.py
This script never runs on the GPU box and nothing under tests/ imports it.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_goldens as mg  # noqa: E402  (puts the repository root and tests/ on sys.path)

NUM_LABELS, NUM_SCENE, BATCH = 7, 6, 4          # action classes of the unified head, scene classes behind them; 4 samples per batch: accuracies exact in fp32
MERGE_CLASSES, MERGE_VIDEOS = 8, 7              # three classes beyond five: top-5 is not trivial


def accuracy(output, target, topk=(1,)):
    """timm 0.4.12 timm/utils/metrics.py"""
    maxk = max(topk)
    batch_size = target.size(0)
    _, pred = output.topk(maxk, 1, True, True)
    pred = pred.t()
    correct = pred.eq(target.reshape(1, -1).expand_as(pred))
    return [correct[:k].reshape(-1).float().sum(0) * 100. / batch_size for k in topk]


class Replay(nn.Module):
    """returns the next of the given outputs at every call"""

    def __init__(self, outputs):
        super().__init__()
        self.outputs, self.calls = list(outputs), 0

    def forward(self, x, return_attn=False):
        self.calls += 1
        return self.outputs[self.calls - 1]


def scene_case(eng):
    g = torch.Generator().manual_seed(7301)
    batches, student, teacher = [], [], []
    for b in range(2):
        z = torch.randn(BATCH, NUM_LABELS + NUM_SCENE, generator=g)
        t = torch.randn(BATCH, NUM_SCENE, generator=g)
        for i in range(BATCH):          # most samples: the student agrees with the teacher (top-1), or nearly (second largest); the rest is noise
            if (b * BATCH + i) % 3 != 2:
                z[i, NUM_LABELS + int(t[i].argmax())] += 3.0 if (b + i) % 2 == 0 else 0.9
        ids = ["vid%02d" % (b * BATCH + i) for i in range(BATCH)]
        chunk = torch.tensor([(b + i) % 5 for i in range(BATCH)])
        split = torch.tensor([(b * BATCH + i) % 3 for i in range(BATCH)])
        batches.append((torch.zeros(BATCH, 1), torch.zeros(BATCH, dtype=torch.long), ids, chunk, split))
        student.append(z); teacher.append(t)
    model = Replay([(None, (None, z, None), None) for z in student])
    scene_model = Replay([(None, t) for t in teacher])
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "0.txt")
        stats = eng.final_test_with_scene_label(batches, model, scene_model, "cpu", path, num_labels=NUM_LABELS)
        text = open(path).read()
    assert model.calls == 2 and scene_model.calls == 2
    assert 0.0 < stats["acc1"] < stats["acc5"] < 100.0, stats
    print("[scene] returned", stats, "first line", repr(text.split("\n")[0]))
    return {"num_labels": NUM_LABELS, "ids": [b[2] for b in batches], "chunk": [b[3].tolist() for b in batches], "split": [b[4].tolist() for b in batches],
            "student_scene_logits": [z.tolist() for z in student], "teacher_logits": [t.tolist() for t in teacher],
            "file": text, "stats": {k: float(v) for k, v in stats.items()}}


def merge_case(eng):
    """7 videos, 2 ranks; video 6 is seen by rank 0 only; (chunk 4, split 2) of video 3 appears on both ranks, the second time voting for a wrong class strongly
    enough to change the video's prediction if it were counted"""
    rng = np.random.RandomState(7302)
    labels = [int(rng.randint(0, MERGE_CLASSES)) for _ in range(MERGE_VIDEOS)]
    texts = []
    for rank in range(2):
        lines = ["tensor(0.), tensor(0.)\n"]
        for v in range(MERGE_VIDEOS):
            if v == 6 and rank == 1:
                continue
            for view in range(3):
                chunk, split = (2 * view + rank) % 5, view
                z = rng.randn(MERGE_CLASSES).astype(np.float32) * 1.5
                if v == 3:
                    z = z * np.float32(0.05)
                    z[labels[v]] += 0.5                          # right, by a margin that one confident wrong view overturns
                elif v % 3 == 0:
                    z[labels[v]] += 4.0                          # right
                elif v % 3 == 1:
                    z[labels[v]] += 1.0                          # near the top
                if v == 3 and rank == 1 and view == 0:
                    chunk, split = 4, 2                          # rank 0 wrote (4, 2) for view 2 of this video: this one is dropped
                    z[:] = 0.0
                    z[(labels[v] + 1) % MERGE_CLASSES] = 30.0
                lines.append("{} {} {} {} {}\n".format("vid%d" % v, str(z.tolist()), str(labels[v]), str(chunk), str(split)))
        texts.append("".join(lines))
    with tempfile.TemporaryDirectory() as d:
        for rank, t in enumerate(texts):
            open(os.path.join(d, "%d.txt" % rank), "w").write(t)
        top1, top5 = eng.merge(d, 2)
        # the duplicate matters: with its key changed (so that it is counted) the result differs
        open(os.path.join(d, "1.txt"), "w").write(texts[1].replace("] %d 4 2\n" % labels[3], "] %d 3 2\n" % labels[3]))
        other = eng.merge(d, 2)
    assert texts[0].count("vid3 ") == 3 and texts[0].count("] %d 4 2\n" % labels[3]) >= 1 and texts[1].count("] %d 4 2\n" % labels[3]) == 1
    assert (float(top1), float(top5)) != (float(other[0]), float(other[1])), (top1, top5, other)
    assert 0.0 < top1 < top5 < 100.0, (top1, top5)
    print("[merge] top1 %r top5 %r (with the duplicate counted: %r)" % (top1, top5, other))
    return {"files": texts, "top1": float(top1), "top5": float(top5)}


def main():
    mg.install_reference()
    sys.modules["timm.utils"].accuracy = accuracy
    import engine.engine_for_slot as eng
    fx = {"scene": scene_case(eng), "merge": merge_case(eng)}
    path = os.path.join(mg.ROOT, "tests", "golden", "eval_engine.json")
    with open(path, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
