"""The detections' model (csrc/detect.h) in plain numpy / Python integers, independently of the C code: class, candidate,
order, cap, greedy suppression per class.  The model is this project's own (the reference draws every window that fires);
it is stated once in detect.h and restated here.  Python integers are unbounded: the IoU compare needs no care."""
import numpy as np

MAX_CANDIDATES = 4096
FIELDS = 8


def decode_class(scores):
    """the decode's class of each row of ``scores`` [n, ncls]: the first strict maximum, floored at 0"""
    s = np.asarray(scores, dtype=np.int64)
    best = np.argmax(s, axis=1)  # (numpy's argmax returns the first maximum)
    return np.where(s[np.arange(len(s)), best] > 0, best, 0)


def suppresses(a, b, num, den):
    """whether kept box ``a`` suppresses box ``b``: IoU(a, b) > num / den, in integers"""
    iw = min(a[2], b[2]) - max(a[0], b[0])
    ih = min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return False
    inter = int(iw) * int(ih)
    union = int(a[2] - a[0]) * int(a[3] - a[1]) + int(b[2] - b[0]) * int(b[3] - b[1]) - inter
    return inter * den > num * union


def detect_frame(boxes, scores, class_mask, by_score, min_score, iou, max_candidates, max_det):
    """one frame -> (dets [k, 8] int32, n_candidates)"""
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.int64).reshape(len(boxes), -1)
    num, den = iou
    if by_score:
        only = [k for k in range(64) if (class_mask >> k) & 1]
        assert len(only) == 1
        cls = np.full(len(boxes), only[0], dtype=np.int64)
    else:
        cls = decode_class(scores)
    own = scores[np.arange(len(boxes)), cls]
    cand = [i for i in range(len(boxes)) if (class_mask >> int(cls[i])) & 1 and own[i] > min_score]
    n_candidates = len(cand)
    cand.sort(key=lambda i: (-int(own[i]), i))
    cand = cand[:max_candidates]
    kept = []
    for i in cand:
        if len(kept) == max_det:
            break
        if any(cls[k] == cls[i] and suppresses(boxes[k], boxes[i], num, den) for k in kept):
            continue
        kept.append(i)
    dets = np.array([[boxes[i][0], boxes[i][1], boxes[i][2], boxes[i][3], cls[i], own[i], i, boxes[i][2] - boxes[i][0]] for i in kept],
                    dtype=np.int32).reshape(-1, FIELDS)
    return dets, n_candidates


def detect(boxes, scores, class_mask, by_score=0, min_score=-32769, iou=(1, 2), max_candidates=MAX_CANDIDATES, max_det=64):
    """``scores`` [F, n, ncls] -> (dets int32 [F, max_det, 8] with zero rows past the count, counts [F], n_candidates [F])"""
    scores = np.asarray(scores)
    frames = scores.shape[0]
    dets = np.zeros((frames, max_det, FIELDS), np.int32)
    counts, ncand = np.zeros(frames, np.int32), np.zeros(frames, np.int32)
    for f in range(frames):
        d, ncand[f] = detect_frame(boxes, scores[f], class_mask, by_score, min_score, iou, max_candidates, max_det)
        counts[f] = len(d)
        dets[f, :len(d)] = d
    return dets, counts, ncand
