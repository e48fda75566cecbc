"""The oracle of the line-order tests: the line model of read_page in plain Python, written from its statement (DESIGN.md
9, include/bnn_mi355x.h), apart from csrc/page.cpp.

Input: boxes (l, u, r, b; right and lower exclusive) and first pixels f of the components kept by min_pixels.
  1  visit in ascending (u, f)
  2  every line has a band [top, bottom); a visited component of height h = b - u joins the line with the largest
     ov = min(b, bottom) - max(u, top) among the lines with 2 ov >= min(h, bottom - top), on a tie the line created first;
     the band's bottom becomes max(bottom, b); no line qualifies: a new line [u, b)
  3  lines are numbered in creation order
  4  inside a line: ascending (l, u, f)
  5  output: line 0, line 1, ...
  6  gap[i] = 1 iff word_gap > 0, glyph i is not the first of its line, and l_i - max(r of the earlier glyphs of its line)
     >= word_gap
Ties that real components cannot have (equal (u, f), equal (l, u, f)) go by input index: Python's sort is stable.
"""


def order_lines(boxes, first, word_gap=0):
    """-> (order, line, gap): order[i] is the input index of output glyph i"""
    boxes = [tuple(int(v) for v in b) for b in boxes]
    first = [int(f) for f in first]
    lines = []  # [top, bottom, [members]]
    for i in sorted(range(len(boxes)), key=lambda i: (boxes[i][1], first[i])):
        _, u, _, b = boxes[i]
        best, best_ov = None, None
        for ln in lines:
            top, bottom = ln[0], ln[1]
            ov = min(b, bottom) - max(u, top)
            if 2 * ov >= min(b - u, bottom - top) and (best is None or ov > best_ov):
                best, best_ov = ln, ov
        if best is None:
            lines.append([u, b, [i]])
        else:
            best[1] = max(best[1], b)
            best[2].append(i)
    order, line, gap = [], [], []
    for k, (_, _, members) in enumerate(lines):
        right = None
        for i in sorted(members, key=lambda i: (boxes[i][0], boxes[i][1], first[i])):
            order.append(i)
            line.append(k)
            gap.append(1 if word_gap > 0 and right is not None and boxes[i][0] - right >= word_gap else 0)
            right = boxes[i][2] if right is None else max(right, boxes[i][2])
    return order, line, gap


def text_of(names, line, gap):
    """the string read_text makes: lines joined with a newline, a space where gap is set"""
    out = []
    for i, name in enumerate(names):
        if i and line[i] != line[i - 1]:
            out.append("\n")
        elif gap[i]:
            out.append(" ")
        out.append(name)
    return "".join(out)
