// Executor objects: what snapshots (snapshot.hip), digests (digest.hip), world
// views (world_view.hip), world writes (world_write.hip), world reduces
// (world_reduce.hip), entity gathers (entity_gather.hip), entity scatters
// (entity_scatter.hip), ray queries (ray_query.hip), box queries
// (box_query.hip), contact queries (contact_query.hip) and shape queries
// (shape_query.hip) share on the host
// (what the last nine share as step-batched objects is in
// step_batch.hpp, what the last four share besides in tree_query.hpp).  An
// executor object
// is a record with device memory of its own, made by mwhip_<kind>_create, named
// by a handle, used through mwhip_<kind>_* and freed by mwhip_<kind>_destroy or
// with its executor.  Host code only.  Not a header to include on its own:
// exec_internal.hpp includes it in front of mwhip_exec (which holds one table
// per kind) and behind what it uses of that file, MWHIP_RT and fail().  Not
// installed.
#pragma once
#include "runtime_internal.hpp"     // mwhip.h (mwhip_digest_column), the HIP runtime

#include <atomic>
#include <cstdint>
#include <memory>
#include <unordered_map>
#include <vector>

struct mwhip_exec;

// One kind's records by handle.  The table owns them; a record frees its device
// and pinned memory in its destructor.  Handles are unique in the process (one
// counter per kind): one of another executor is never found.
template <typename Rec>
class ExecObjectTable {
public:
    ExecObjectTable() = default;
    ExecObjectTable(const ExecObjectTable &) = delete;
    ExecObjectTable &operator=(const ExecObjectTable &) = delete;
    ~ExecObjectTable() { clear(); }

    Rec *find(uint64_t handle) const
    {
        auto it = recs_.find(handle);
        return it == recs_.end() ? nullptr : it->second;
    }

    // takes the record over, gives it its handle (Rec::handle) and returns it
    uint64_t insert(std::unique_ptr<Rec> rec)
    {
        static std::atomic<uint64_t> next { 1 };
        // (runtime.hip destroys executors without knowing the record types)
        if (delete_ == nullptr) delete_ = [](Rec *r) { delete r; };
        const uint64_t handle = next.fetch_add(1);
        rec->handle = handle;
        recs_[handle] = rec.release();
        return handle;
    }

    void erase(uint64_t handle)
    {
        auto it = recs_.find(handle);
        if (it == recs_.end()) return;
        delete_(it->second);
        recs_.erase(it);
    }

    void clear()
    {
        for (auto &kv : recs_) {
            delete_(kv.second);
        }
        recs_.clear();
    }

private:
    std::unordered_map<uint64_t, Rec *> recs_;
    void (*delete_)(Rec *) = nullptr;   // set by the first insert
};

// The record behind a handle; nullptr without an executor, so that an entry
// point can look its object up before anything else.
template <typename Rec>
inline Rec *findObject(const ExecObjectTable<Rec> *table, uint64_t handle)
{
    return table == nullptr ? nullptr : table->find(handle);
}

// -3, "<kind> N is not one of this executor's"
inline int unknownObject(const char *kind, uint64_t handle)
{
    return fail(-3, "%s %llu is not one of this executor's", kind,
                (unsigned long long)handle);
}

// The column list of a create call, resolved: every entry names a registered
// archetype and a component it has, and no (archetype, component) pair is
// listed twice -- otherwise -2 with `what` (the entry point) in front of the
// text, before anything is allocated.  out[p] belongs to columns[p].
struct ResolvedColumn {
    int column = -1;                // in the table
    void *const *slot = nullptr;    // &hdr->columns[column] on the device: where the
                                    // column's base address is read (the sort swaps
                                    // a column with its twin); never read here
    uint32_t cellBytes = 0;
};
MWHIP_RT int resolveColumns(mwhip_exec *exec, const char *what,
                            const mwhip_digest_column *columns, uint32_t n,
                            std::vector<ResolvedColumn> &out);
      // (runtime.hip)

// A create call ran out of device memory: the half-made record goes (its
// destructor frees what it had), the HIP error is not left for the next launch
// check to find, and the call returns -10 with the message given (a literal
// format, checked like any other of fail()).
template <typename Rec>
inline void dropHalfMade(std::unique_ptr<Rec> &rec)
{
    (void)hipGetLastError();
    rec.reset();
}
#define CREATE_FAILED(rec, ...) (dropHalfMade(rec), fail(-10, __VA_ARGS__))

// The end of an entry point that queued work on the executor's stream (rc: what
// queueing it returned): the _async forms return at once, the others wait.
MWHIP_RT int finishQueued(mwhip_exec *exec, int rc, bool wait);
      // (runtime.hip)
