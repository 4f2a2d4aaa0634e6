"""Generates tests/golden/kit_splits_golden.json by IMPORTING the reference's own ``get_data_splits``
(sings/rec/datasets/Customdataset.py:31-42, read-only at /root/reference) in the build container, and copies three files of the
reference's training kit ``examples/training_kits/f_2`` -- data its programs read -- beside it; only inputs and outputs ship.

    python tests/golden/gen_kit_golden.py

The module imports cv2, tqdm, loguru and the reference's own graphics / constants modules at its top for code that is not used here:
whichever is absent is stubbed.  ``get_data_splits`` only takes the length of its argument: for every length 10 .. 400 the golden
holds (first, step, count) of the val list, which is a slice; the train list is the rest (below 10 the rule divides by zero).  The
kit's files: two masks (7 416 and 4 891 bytes: 8-bit grey, one IDAT, every row of filter type Sub, written by cv2) and the smallest
image (165 722 bytes: 8-bit RGB, 21 IDAT chunks).
"""
import importlib
import importlib.util
import json
import os
import shutil
import sys
import types

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

for name, attrs in (("cv2", ()), ("tqdm", ("tqdm",)), ("loguru", ("logger",)), ("sings", ()), ("sings.rec", ()), ("sings.rec.utils", ()),
                    ("sings.rec.utils.graphics", ("get_projection_matrix", "get_projection_matrix_center")), ("sings.rec.defaults", ()),
                    ("sings.rec.defaults.constants", ("DATA_PATH",))):
    try:
        importlib.import_module(name)
    except ImportError:
        stub = types.ModuleType(name)
        for a in attrs:
            setattr(stub, a, types.SimpleNamespace())
        sys.modules[name] = stub
spec = importlib.util.spec_from_file_location("ref_customdataset", os.path.join(REF, "sings/rec/datasets/Customdataset.py"))
ref = importlib.util.module_from_spec(spec); spec.loader.exec_module(ref)

# The val list is a slice, ``range(n)[offset::length]``, and the train list the other frames in ascending order: both are checked here
# for every length, so (first, step, count) of the val list says everything the two lists say.
rows = []
for n in range(10, 401):
    train, val = ref.get_data_splits([None] * n)
    first, step = val[0], (val[1] - val[0] if len(val) > 1 else n)
    assert list(val) == list(range(first, n, step)) and list(train) == sorted(set(range(n)) - set(val))
    rows.append([first, step, len(val)])
dst = os.path.join(ROOT, "tests", "golden", "kit_splits_golden.json")
with open(dst, "w") as f:
    f.write('{"lengths": [10, 400], "train": "the frames not in val, ascending",\n "val_first_step_count": [\n')
    f.write(",\n".join("  " + ", ".join(json.dumps(r, separators=(",", ":")) for r in rows[i:i + 16]) for i in range(0, len(rows), 16)))
    f.write("\n ]}\n")
print("wrote", dst, os.path.getsize(dst), "bytes")

KIT = os.path.join(REF, "examples", "training_kits", "f_2")
for src, name in (("masks/000000.png", "kit_mask_000000.png"), ("masks/000040.png", "kit_mask_000040.png"),
                  ("images/000040.png", "kit_image_000040.png")):
    shutil.copyfile(os.path.join(KIT, src), os.path.join(ROOT, "tests", "golden", name))
    print("copied", name, os.path.getsize(os.path.join(ROOT, "tests", "golden", name)), "bytes")
