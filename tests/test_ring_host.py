"""The ring of both device replay stores (rlzero_amd/csrc/rz_ring.h: rz_replay.hip's positions, rz_mz_replay.hip's episodes) on the
CPU, against a model that knows no modular arithmetic about items: an array of `capacity` cells into which the items of every add
are written ONE BEHIND THE OTHER, each over whatever lies in its cell, read back as the list of (slot, item) pairs it holds -- the
newest `capacity` items.

A driver with its own main is compiled against the header with ROCm's clang++ (by tests/host_driver.py),
once plain and once with -fsanitize=address,undefined -fno-sanitize-recover=all, and run as a stand-alone program over a sequence of
add sizes.  After EVERY add it reports the ticket before and after, skip(kept), oldest(), cursor, count, stored, slot(t) of every
item of the add that gets a slot and window_start(first) of every item held; all of it is compared with the model, and no two items
of one add may share a slot.  The sequences hold adds of 0, 1, exactly the capacity, the capacity + 1 and several times the
capacity, which take the cursor round the ring five times, for capacities 1, 2, 7 and 2^24 (the largest a store takes); the three
small capacities go on with runs of small adds that take it round dozens of times more."""
import os

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the repository on sys.path)
import host_driver

STATE_WORDS = 9

DRIVER = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rz_ring.h"

template <typename T>
static std::vector<T> load(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<T> v((size_t)bytes / sizeof(T));
    if (bytes && fread(v.data(), 1, (size_t)bytes, f) != (size_t)bytes) exit(2);
    fclose(f);
    return v;
}

// ring script.i64 [capacity, kept of add 0, kept of add 1, ..] -> state.i64 [adds][9], slots.i32: per add slot(t) of t = skip .. kept - 1,
// then window_start(first) of first = 0 .. count - 1
int main(int argc, char **argv) {
    if (argc != 4) return 4;
    const std::vector<int64_t> script = load<int64_t>(argv[1]);
    if (script.empty() || script[0] < 1 || script[0] > (1LL << 24)) return 4;
    FILE *state = fopen(argv[2], "wb"), *slots = fopen(argv[3], "wb");
    if (!state || !slots) return 2;
    rz_ring ring;
    ring.capacity = script[0];
    std::vector<int32_t> out;
    for (size_t step = 1; step < script.size(); ++step) {
        const long long kept = script[step];
        const long long before = ring.ticket(), skip = ring.skip(kept);
        out.clear();
        for (long long t = skip; t < kept; ++t) out.push_back((int32_t)ring.slot(t));
        ring.commit(kept);
        for (long long first = 0; first < ring.count; ++first) out.push_back((int32_t)ring.window_start(first));
        const int64_t row[9] = {before, ring.ticket_current(before) ? 1 : 0, skip, ring.oldest(), ring.cursor, ring.count, ring.stored, ring.ticket(),
                                ring.ticket_current(ring.ticket()) ? 1 : 0};
        if (fwrite(row, sizeof(int64_t), 9, state) != 9) return 2;
        if (!out.empty() && fwrite(out.data(), sizeof(int32_t), out.size(), slots) != out.size()) return 2;
    }
    if (fclose(state) != 0 || fclose(slots) != 0) return 2;
    return 0;
}
'''


class Model(object):
    """`capacity` cells; the items 0, 1, 2, .. of all adds are written one behind the other, round and round."""

    def __init__(self, capacity):
        self.cells = np.full(capacity, -1, dtype=np.int64)
        self.next, self.stored = 0, 0

    def add(self, kept):
        done = 0
        while done < kept:   # a run up to the last cell, then on from the first: item by item, in whole runs
            n = min(kept - done, len(self.cells) - self.next)
            self.cells[self.next:self.next + n] = np.arange(self.stored + done, self.stored + done + n)
            self.next = (self.next + n) % len(self.cells)
            done += n
        self.stored += kept

    def pairs(self):
        """The (slot, item) pairs held, oldest item first -> (slots int64 [count], items int64 [count])."""
        slots = np.flatnonzero(self.cells >= 0)
        items = self.cells[slots]
        assert len(items) == min(self.stored, len(self.cells))
        if len(items):   # the newest `capacity` items, each once: stored - count .. stored - 1
            by_age = np.full(len(items), -1, dtype=np.int64)
            by_age[items - (self.stored - len(items))] = slots
            assert (by_age >= 0).all()
            slots, items = by_age, np.arange(self.stored - len(items), self.stored)
        return slots, items


drv = host_driver.fixture('ring', DRIVER)


def run_ring(drv, capacity, adds):
    """-> (state int64 [adds][9], slots int32) of the plain build; the sanitized build ran without a report and wrote the same bytes."""
    state, slots = drv.same(drv.write([np.array([capacity] + list(adds), dtype=np.int64)]), 2)
    state = np.fromfile(state, dtype=np.int64).reshape(len(adds), STATE_WORDS)
    # (at 2^24 slots an add's report is 128 MB: mapped, not read into memory at once)
    return state, np.memmap(slots, dtype=np.int32, mode='r') if os.path.getsize(slots) else np.zeros(0, dtype=np.int32)


def sequences(capacity):
    """The adds of one run: 0, 1, exactly the capacity, the capacity + 1, several times the capacity, and between them small adds; for
    the small capacities also a long run of adds of 0 .. capacity + 2 that takes the cursor round the ring dozens of times."""
    c = capacity
    adds = [0, 1, c, c + 1, 3 * c + 5]   # (the cursor ends at 7 modulo c, five times round)
    if c <= 7:
        rng = np.random.RandomState(1000 + c)
        adds += [5, 0, c, 2, 1] + [1] * (3 * c + 1) + [int(v) for v in rng.randint(0, c + 3, size=40 * c)] + [7 * c, c - 1, c, c, 2 * c + 1, 0]
    return adds


@pytest.mark.parametrize('capacity', [1, 2, 7, 1 << 24])
def test_the_ring_holds_the_newest_items_where_the_model_holds_them(drv, capacity):
    adds = sequences(capacity)
    assert {0, 1, capacity, capacity + 1, 3 * capacity + 5} <= set(adds)
    state, slots = run_ring(drv, capacity, adds)
    model, at, wraps, cursor_before = Model(capacity), 0, 0, 0
    for kept, row in zip(adds, state):
        before, current_before, skip, oldest, cursor, count, stored, after, current_after = (int(v) for v in row)
        stored_before = model.stored
        model.add(kept)
        held_slots, held_items = model.pairs()
        # the ticket: the items ever stored; the one taken before an add holds exactly when the add stored nothing
        assert before == stored_before and after == model.stored and current_after == 1
        assert current_before == (1 if kept == 0 else 0)
        assert (cursor, count, stored) == (model.next, len(held_items), model.stored)
        assert oldest == (int(held_slots[0]) if count else cursor)
        # the add's own items: the model still holds the last kept - skip of them, each in the slot the ring named, no slot twice
        mine = held_items >= stored_before
        assert skip == kept - int(mine.sum())
        got = slots[at:at + kept - skip]
        at += kept - skip
        assert len(got) == kept - skip and np.array_equal(got, held_slots[mine])
        assert len(np.unique(got)) == len(got)
        # the read window: held item `first`, oldest first
        windows = slots[at:at + count]
        at += count
        assert len(windows) == count and np.array_equal(windows, held_slots)
        wraps += (cursor_before + kept) // capacity
        cursor_before = cursor
    assert at == len(slots)
    assert wraps > 1   # the cursor went round more than once
