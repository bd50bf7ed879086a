"""The loop-closure candidate source (include/kt_abi.h: kt_loop_db_*) restated in numpy: no GPU, no oracle.

It takes the place of PlaceRecognition::process's dbowInterface->detectLoop() (a DLoopDetector over SURF words with use_nss, alpha = 0.3,
k = 1) and is a definition, not a port of DBoW2 / DLoopDetector: a database of the bootstrap's BRIEF-256 descriptor lists, a score that
counts the query descriptors accepted against an entry under kt_descriptor_match's rule, and DLoopDetector's roles (normalisation by the
previous image, the alpha threshold, islands, temporal consistency) on integers.  All arithmetic is integer, so csrc/kt_loopdb.hip
computes the same values.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from . import loop_match_ref as mref

EMPTY, LOW_REFERENCE, NO_CANDIDATE, NOT_CONSISTENT, DETECTED = range(5)
STATUS_NAMES = ("EMPTY", "LOW_REFERENCE", "NO_CANDIDATE", "NOT_CONSISTENT", "DETECTED")


@dataclass
class DetectParams:                 # kt_loop_db_detect_params and kt_loop_db_detect_params_default
    dislocal: int = 20              # this project's choice: entries newer than newest - dislocal are never candidates
    alpha_num: int = 3              # alpha_num / alpha_den = the reference's alpha = 0.3
    alpha_den: int = 10
    min_score: int = 40             # the caller's 40-match gate: a pair scoring less cannot pass it
    max_gap: int = 3                # this project's choice: ids up to this far apart belong to one island
    consistency: int = 1            # the reference's k = 1


@dataclass
class Result:                       # kt_loop_db_result
    entry: int = 0
    status: int = EMPTY
    candidate: int = -1
    candidate_score: int = 0
    reference_score: int = 0
    island_first: int = -1
    island_last: int = -1
    island_score: int = 0
    n_keypoints: int = 0

    def fields(self) -> tuple:
        return (self.entry, self.status, self.candidate, self.candidate_score, self.reference_score, self.island_first, self.island_last, self.island_score,
                self.n_keypoints)


def score(desc_query: np.ndarray, desc_entry: np.ndarray, prm: mref.Params = mref.Params()) -> int:
    """s(q, e): the query descriptors accepted against the entry (no cross-check); 0 when either is empty"""
    if len(desc_query) == 0 or len(desc_entry) == 0:
        return 0
    idx, _, _ = mref.descriptor_match(np.asarray(desc_query, np.uint32).reshape(-1, 8), np.asarray(desc_entry, np.uint32).reshape(-1, 8), prm)
    return int((idx >= 0).sum())


def scores(desc_query: np.ndarray, entries, prm: mref.Params = mref.Params()) -> np.ndarray:
    """kt_loop_db_scores: int32 [len(entries)]"""
    return np.array([score(desc_query, e, prm) for e in entries], np.int32)


def select(s, prev_island: Optional[Tuple[int, int]], prm: DetectParams = DetectParams()) -> Result:
    """kt_host_loop_db_select (steps 1 - 5): s[e] = s(q, e) for the size entries before the query"""
    s = [int(v) for v in s]
    size = len(s)
    r = Result(entry=size)
    if size == 0:
        return r
    newest = size - 1
    ref = r.reference_score = s[newest]
    if ref < prm.min_score:
        r.status = LOW_REFERENCE
        return r
    cand = [e for e in range(0, newest - prm.dislocal + 1) if s[e] >= prm.min_score and prm.alpha_den * s[e] >= prm.alpha_num * ref]
    if not cand:
        r.status = NO_CANDIDATE
        return r
    islands, run = [], [cand[0]]
    for e in cand[1:]:
        if e - run[-1] <= prm.max_gap:
            run.append(e)
        else:
            islands.append(run)
            run = [e]
    islands.append(run)
    best = min(islands, key=lambda isl: (-sum(s[e] for e in isl), isl[0]))
    top = min(best, key=lambda e: (-s[e], e))
    r.island_first, r.island_last, r.island_score, r.candidate_score = best[0], best[-1], sum(s[e] for e in best), s[top]
    stands = True
    if prm.consistency:
        g = prm.max_gap
        stands = prev_island is not None and prev_island[0] >= 0 and prev_island[0] - g <= best[-1] + g and best[0] - g <= prev_island[1] + g
    r.status = DETECTED if stands else NOT_CONSISTENT
    if stands:
        r.candidate = top
    return r


@dataclass
class Database:                     # kt_loop_db
    max_entries: int
    match: mref.Params = field(default_factory=mref.Params)
    entries: List[np.ndarray] = field(default_factory=list)
    prev_island: Optional[Tuple[int, int]] = None

    def add_descriptors(self, desc: np.ndarray) -> int:
        if len(self.entries) >= self.max_entries:
            raise OverflowError("the database is full")
        desc = np.asarray(desc, np.uint32).reshape(-1, 8)
        assert len(desc) <= self.match.max_keypoints
        self.entries.append(desc.copy())
        return len(self.entries) - 1

    def detect_descriptors(self, desc: np.ndarray, prm: DetectParams = DetectParams()) -> Result:
        """steps 1 - 6 for a query's descriptors"""
        if len(self.entries) >= self.max_entries:
            raise OverflowError("the database is full")
        desc = np.asarray(desc, np.uint32).reshape(-1, 8)
        r = select(scores(desc, self.entries, self.match), self.prev_island, prm)
        r.n_keypoints = len(desc)
        self.prev_island = (r.island_first, r.island_last) if r.island_first >= 0 else None
        self.entries.append(desc.copy())
        return r

    def detect(self, rgb: np.ndarray, depth: np.ndarray, prm: DetectParams = DetectParams()) -> Result:
        """kt_loop_db_detect: the frame's keypoints are loop_match_ref.frame_keypoints'"""
        return self.detect_descriptors(mref.frame_keypoints(rgb, depth, self.match)[2], prm)

    def reset(self) -> None:
        self.entries, self.prev_island = [], None
