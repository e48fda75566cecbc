"""The oracle of the glyph tests: cells 9-13 of LFC-BNN_MNIST_Webcam.ipynb / LFC-BNN_Chars_Webcam.ipynb in plain Pillow,
as the notebooks run them -- greyscale, ImageEnhance.Contrast and .Brightness, the chars notebook's hard threshold, the
80-pixel white border, getbbox of the inverse, crop, Image.resize into 28 x 28 keeping the aspect ratio, the centred paste
on white, the invert and 255 / 1 per pixel.  Nothing here knows how the runtime does it.

Two things are not the notebooks' own:
  * per box: the notebooks handle one glyph per frame; here the enhanced frame is cropped to each box first.
  * the threshold runs before the border is added (the notebook adds the border first).  The border is 255, and
    `p > threshold and 255` keeps 255 for every threshold below 255, so the order shows only at threshold 255, which
    turns the notebook's own border into ink; no record test uses it.
`square_blank=True` keeps the notebooks' square branch as it is (it resizes, forgets the paste and hands the net a blank
record); False pastes the resized glyph, the evident intent.  Status 2 is where Pillow's resize raises ValueError.
"""
import numpy as np
from PIL import Image, ImageEnhance, ImageOps

BORDER = 80
OK, NO_INK, TOO_THIN = 0, 1, 2


def enhance(img, contrast=3, brightness=4.0, threshold=None):
    """cell 9 up to the border -> (the "L" picture the notebooks display, the mean ImageEnhance.Contrast blends with)"""
    from PIL import ImageStat
    img = img.convert("L")
    mean = int(ImageStat.Stat(img).mean[0] + 0.5)
    img = ImageEnhance.Contrast(img).enhance(contrast)
    img = ImageEnhance.Brightness(img).enhance(brightness)
    if threshold is not None and threshold >= 0:
        img = img.point(lambda p: p > threshold and 255)
    return img, mean


def record(frame, filter=None, square_blank=False):
    """cells 9 (the border), 11 and 13 on one enhanced "L" frame -> (784 bytes or None, ink box in frame coordinates, status)"""
    img = ImageOps.expand(frame, border=BORDER, fill="white")
    inverted = ImageOps.invert(img)
    box = inverted.getbbox()
    status = OK
    if box is None:  # no ink: the frame itself (the notebook would fail on crop(None) of nothing; a blank record is meant)
        box = (BORDER, BORDER, BORDER + frame.size[0], BORDER + frame.size[1])
        status = NO_INK
    img_new = img.crop(box)
    ink = tuple(v - BORDER for v in box)
    width, height = img_new.size
    ratio = min((28. / height), (28. / width))
    background = Image.new("RGB", (28, 28), (255, 255, 255))
    kw = {} if filter is None else {"resample": filter}
    try:
        if height == width:
            img_new = img_new.resize((28, 28), **kw)
            if not square_blank:
                background.paste(img_new, (int((28 - img_new.size[0]) / 2), int((28 - img_new.size[1]) / 2)))
        elif height > width:
            img_new = img_new.resize((int(width * ratio), 28), **kw)
            background.paste(img_new, (int((28 - img_new.size[0]) / 2), int((28 - img_new.size[1]) / 2)))
        else:
            img_new = img_new.resize((28, int(height * ratio)), **kw)
            background.paste(img_new, (int((28 - img_new.size[0]) / 2), int((28 - img_new.size[1]) / 2)))
    except ValueError:
        return None, ink, TOO_THIN
    img_data = np.asarray(background)[:, :, 0]
    # (the PNG the notebooks write and read back in between is the identity on uint8)
    smallimg = ImageOps.invert(Image.fromarray(img_data).convert("L"))
    pixel = smallimg.load()
    data = []
    for x in range(0, 28):
        for y in range(0, 28):
            data.append(255 if pixel[y, x] == 255 else 1)
    return np.asarray(data, np.uint8), ink, status


def glyphs(img, boxes=None, contrast=3, brightness=4.0, threshold=None, filter=None, square_blank=False):
    """-> (records [n, 784] with zeros for a status-2 glyph, ink boxes [n, 4] in picture coordinates, status [n])"""
    frame, _ = enhance(img, contrast, brightness, threshold)
    boxes = [(0, 0) + frame.size] if boxes is None else [tuple(int(v) for v in b) for b in boxes]
    recs = np.zeros((len(boxes), 784), np.uint8)
    inks = np.zeros((len(boxes), 4), np.int32)
    status = np.zeros(len(boxes), np.int32)
    for i, b in enumerate(boxes):
        rec, ink, status[i] = record(frame.crop(b), filter, square_blank)
        inks[i] = (b[0] + ink[0], b[1] + ink[1], b[0] + ink[2], b[1] + ink[3])
        if rec is not None:
            recs[i] = rec
    return recs, inks, status


def idx_file(records):
    """the bytes of an idx3 file holding the records (cell 13's header, for any count)"""
    records = np.ascontiguousarray(records, np.uint8).reshape(-1, 784)
    return bytes([0, 0, 8, 3]) + len(records).to_bytes(4, "big") + bytes([0, 0, 0, 28, 0, 0, 0, 28]) + records.tobytes()
