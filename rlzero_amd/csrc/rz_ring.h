// rz_ring.h -- the ring both device replay stores keep their items in (rz_replay.hip: positions; rz_mz_replay.hip: episodes), once:
// where the next item goes, which items are held, which of an add's items get a slot, and the ticket that ties a Reanalyse result
// to the store it was drawn from.  Host bookkeeping only, four integers: plain C++ with no attribute at all, no HIP include, so
// that the CPU holds it to a list of the newest `capacity` items (tests/test_ring_host.py).  The kernels get `cursor`, `oldest()`
// and `skip(kept)` as arguments and reduce modulo the capacity themselves.
#pragma once

struct rz_ring {
    long long capacity = 1;   // slots (>= 1)
    long long cursor = 0;     // next slot written
    long long count = 0;      // items held: the newest min(stored, capacity)
    long long stored = 0;     // items ever stored

    // the slot of the oldest item held
    long long oldest() const { return ((cursor - count) % capacity + capacity) % capacity; }
    // An add of `kept` items, item t = 0 .. kept - 1 in order: the first skip(kept) get no slot -- of more items than slots only the
    // last `capacity` are written, so no two items of one add share a slot -- and item t >= skip(kept) goes to slot(t).
    long long skip(long long kept) const { return kept > capacity ? kept - capacity : 0; }
    long long slot(long long t) const { return (cursor + t) % capacity; }
    void commit(long long kept) {
        cursor = (cursor + kept) % capacity;
        count = count + kept > capacity ? capacity : count + kept;
        stored += kept;
    }
    // the slot of held item `first` (0 = the oldest): a read of n items from there runs to the ring's end, then from its start
    long long window_start(long long first) const { return (oldest() + first) % capacity; }
    // The ticket: the number of items EVER stored.  A count, not the cursor: the cursor returns to the same slot after `capacity`
    // items, the count never does.  A result may be written back only while nothing was stored since its ticket was taken.
    long long ticket() const { return stored; }
    bool ticket_current(long long t) const { return t == stored; }
};
