"""An independent numpy restatement of the part-segmentation metrics of the reference's `validate`
(tools/runner_unify_seg.py:301-367): per-shape loops, np.argmax, np.mean, the reference's own category order.  The tests hold
utils.evaluate.SegMetric (CPU and HIP paths) and the validate_seg protocols against it."""
import numpy as np

# reference tools/runner_unify_seg.py:79-82, in its dict order
SEG_CLASSES = {'Earphone': [16, 17, 18], 'Motorbike': [30, 31, 32, 33, 34, 35], 'Rocket': [41, 42, 43], 'Car': [8, 9, 10, 11],
               'Laptop': [28, 29], 'Cap': [6, 7], 'Skateboard': [44, 45, 46], 'Mug': [36, 37], 'Guitar': [19, 20, 21], 'Bag': [4, 5],
               'Lamp': [24, 25, 26, 27], 'Table': [47, 48, 49], 'Airplane': [0, 1, 2, 3], 'Pistol': [38, 39, 40],
               'Chair': [12, 13, 14, 15], 'Knife': [22, 23]}


def reference_metrics(batches, num_part=50):
    """batches: [(logp (B, N, P) float32 array, target (B, N) int array)] -> dict with the reference's four metrics, 'category_iou',
    and what the tests compare exactly: 'pred' [(B, N) int64 per batch], 'shape_iou' (shapes in batch order), 'correct', 'seen',
    'part_seen', 'part_correct'."""
    seg_label_to_cat = {label: cat for cat, labels in SEG_CLASSES.items() for label in labels}
    total_correct = total_seen = 0
    total_seen_class = [0 for _ in range(num_part)]
    total_correct_class = [0 for _ in range(num_part)]
    shape_ious = {cat: [] for cat in SEG_CLASSES.keys()}
    preds, in_order = [], []
    for logits_all, target in batches:
        B, N = target.shape
        pred = np.zeros((B, N), dtype=np.int64)
        for i in range(B):
            cat = seg_label_to_cat[target[i, 0]]
            pred[i, :] = np.argmax(logits_all[i][:, SEG_CLASSES[cat]], 1) + SEG_CLASSES[cat][0]
        preds.append(pred)
        total_correct += int(np.sum(pred == target))
        total_seen += B * N
        for l in range(num_part):
            total_seen_class[l] += int(np.sum(target == l))
            total_correct_class[l] += int(np.sum((pred == l) & (target == l)))
        for i in range(B):
            segp, segl = pred[i, :], target[i, :]
            cat = seg_label_to_cat[segl[0]]
            part_ious = [0.0 for _ in range(len(SEG_CLASSES[cat]))]
            for l in SEG_CLASSES[cat]:
                if (np.sum(segl == l) == 0) and (np.sum(segp == l) == 0):
                    part_ious[l - SEG_CLASSES[cat][0]] = 1.0
                else:
                    part_ious[l - SEG_CLASSES[cat][0]] = np.sum((segl == l) & (segp == l)) / float(np.sum((segl == l) | (segp == l)))
            shape_ious[cat].append(np.mean(part_ious))
            in_order.append(np.mean(part_ious))
    with np.errstate(divide='ignore', invalid='ignore'):
        all_shape_ious = [iou for cat in shape_ious for iou in shape_ious[cat]]
        cat_iou = {cat: np.mean(v) if v else np.float64('nan') for cat, v in shape_ious.items()}
        return {'accuracy': total_correct / float(total_seen) if total_seen else float('nan'),
                'class_avg_accuracy': float(np.mean(np.array(total_correct_class) / np.array(total_seen_class, dtype=float))),
                'class_avg_iou': float(np.mean(list(cat_iou.values()))),
                'inctance_avg_iou': float(np.mean(all_shape_ious)) if all_shape_ious else float('nan'),
                'category_iou': {k: float(v) for k, v in cat_iou.items()},
                'pred': preds, 'shape_iou': np.array(in_order, dtype=np.float64), 'correct': total_correct, 'seen': total_seen,
                'part_seen': np.array(total_seen_class), 'part_correct': np.array(total_correct_class)}


def close(a, b, rel=1e-12):
    """Equal within `rel` relative, NaN equal to NaN."""
    a, b = float(a), float(b)
    if a != a or b != b:
        return a != a and b != b
    return abs(a - b) <= rel * max(abs(a), abs(b), 1e-300)


def assert_metrics_match(got, want, rel=1e-12):
    for k in ('accuracy', 'class_avg_accuracy', 'class_avg_iou', 'inctance_avg_iou'):
        assert close(got[k], want[k], rel), (k, got[k], want[k])
    assert set(got['category_iou']) == set(want['category_iou'])
    for k, v in want['category_iou'].items():
        assert close(got['category_iou'][k], v, rel), (k, got['category_iou'][k], v)


def planted_batch(B, N, seed, num_part=50, nan_rows=True, ties=True):
    """(logp (B, N, P) float32, target (B, N) int64): log-softmax of random logits, targets drawn inside each shape's category (the
    first one decides it) with a few foreign labels, the true part raised on about half the points; then exact ties and NaN rows."""
    rng = np.random.default_rng(seed)
    cats = list(SEG_CLASSES.values())
    logits = rng.standard_normal((B, N, num_part)).astype(np.float32)
    target = np.zeros((B, N), dtype=np.int64)
    for i in range(B):
        parts = cats[rng.integers(len(cats))]
        use = parts[:max(1, rng.integers(1, len(parts) + 1))]          # some parts absent from the shape
        target[i] = rng.choice(use, N)
        foreign = rng.random(N) < 0.05
        target[i, foreign] = rng.integers(0, num_part, int(foreign.sum()))
        target[i, 0] = use[0]
        boost = rng.random(N) < 0.5
        logits[i, np.arange(N)[boost], target[i, boost]] += 3.0
    x = logits - logits.max(-1, keepdims=True)
    logp = (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)
    if ties and N >= 4:
        for i in range(B):
            parts = next(p for p in cats if target[i, 0] in p)
            logp[i, 1, parts] = -1.5                                      # all equal: the first part
            if len(parts) > 1:
                logp[i, 2, parts[-1]] = logp[i, 2, parts[0]] = logp[i, 2, parts].max() + 0.5     # a tie of the first and last
    if nan_rows and N >= 6:
        for i in range(B):
            parts = next(p for p in cats if target[i, 0] in p)
            logp[i, 3, parts] = np.nan                                    # all NaN: the first part
            logp[i, 4, parts[-1]] = np.nan                                # one NaN: it wins
            if len(parts) > 2:
                logp[i, 5, parts[1]] = logp[i, 5, parts[2]] = np.nan      # two NaNs: the first
    return logp, target
