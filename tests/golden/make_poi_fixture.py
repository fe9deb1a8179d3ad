"""Regenerates tests/golden/poi_tract_counts.npy from the reference's miscs/POI_tract.pickle:

    python tests/golden/make_poi_fixture.py <reference checkout>/miscs/POI_tract.pickle

The pickle (written by Python 2) holds ordKey, the 801 tract ids in the order the reference evaluates them, and tract_poi, id -> {category: count} for the 792
tracts that have a POI.  The fixture is int32 [801 x 11]: the tract id, then the ten counts in the header order of generatePairWiseGT
(P/embeddingEvaluation_tract.py:71-73), 0 for a category or a tract the pickle lacks (:76-84).  Data the reference's programs read, no program text.
Rows 361, 409, 472, 511, 557, 561, 562, 597 and 655 are all-zero: the zero vectors of the pairwise evaluation's rule (include/dge.h)."""
import os
import pickle
import sys

import numpy as np

HEADER = ["Food", "Residence", "Travel", "Arts & Entertainment", "Outdoors & Recreation", "College & Education", "Nightlife", "Professional", "Shops", "Event"]

with open(sys.argv[1], "rb") as fin:
    ord_key = pickle.load(fin, encoding="latin1")
    tract_poi = pickle.load(fin, encoding="latin1")
a = np.zeros((len(ord_key), 11), np.int32)
for i, k in enumerate(ord_key):
    a[i, 0] = k
    for j, p in enumerate(HEADER):
        a[i, 1 + j] = tract_poi.get(k, {}).get(p, 0)
np.save(os.path.join(os.path.dirname(os.path.abspath(__file__)), "poi_tract_counts.npy"), a)
print("wrote poi_tract_counts.npy:", a.shape, "zero rows", np.flatnonzero((a[:, 1:] == 0).all(axis=1)).tolist())
