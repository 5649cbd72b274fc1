// Cross-stream event waits of a two-stream schedule, as pure host bookkeeping (no HIP, no plan handle): what `run_schedule`
// (plan_runtime.cpp) turns into hipStreamWaitEvent calls and what `cp_schedule_waits` hands to plan tooling and to the tests.
// The Python twin is engine.capture_waits (over Engine.dependencies).
#ifndef CP_SCHEDULE_WAITS_H
#define CP_SCHEDULE_WAITS_H
#include <vector>

// Op i runs on capture stream streams[i] != 0 ? 1 : 0 and names nptr[i] buffers, bufids (flat, op after op): the activation-buffer
// id behind each pointer (instance base already added), -1 for constants / NULL.  The pointer at out_index[i] is the one it writes.
// An op follows the last writer of every buffer it names, and the last writer's readers of the buffer it writes (RAW / WAW / WAR
// per buffer).  Streams are FIFO, so an op waits only for the youngest such op of the OTHER stream, and only when its own stream has
// not waited for that op or a younger one already.  wait_for[i] = that op, or -1.  Returns false for an id outside [-1, nbuf).
inline bool schedule_waits(int n_ops, const int* streams, const int* nptr, const int* bufids, const int* out_index, int nbuf,
                           std::vector<int>& wait_for)
{
    std::vector<int> last_writer(nbuf > 0 ? nbuf : 0, -1);
    std::vector<std::vector<int>> readers(nbuf > 0 ? nbuf : 0);
    int waited[2] = {-1, -1};
    wait_for.assign(n_ops > 0 ? n_ops : 0, -1);
    const int* ids = bufids;
    for (int i = 0; i < n_ops; ids += nptr[i], ++i) {
        const int me = streams[i] ? 1 : 0, other = me ^ 1;
        int need = -1;                                   // youngest op of the other stream this one must follow
        auto follow = [&](int j) { if (j >= 0 && (streams[j] ? 1 : 0) == other && j > need) need = j; };
        for (int k = 0; k < nptr[i]; ++k) {
            const int b = ids[k];
            if (b < 0) continue;
            if (b >= nbuf) return false;
            follow(last_writer[b]);
            if (k == out_index[i]) for (int j : readers[b]) follow(j);
        }
        if (need > waited[me]) {
            wait_for[i] = need;
            waited[me] = need;
        }
        for (int k = 0; k < nptr[i]; ++k) {
            const int b = ids[k];
            if (b < 0) continue;
            if (k == out_index[i]) { last_writer[b] = i; readers[b].clear(); }
            else readers[b].push_back(i);
        }
    }
    return true;
}

#endif
