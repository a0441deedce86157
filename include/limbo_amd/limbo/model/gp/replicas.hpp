// limbo/model/gp/replicas.hpp — the engine handle of a drop-in model::GP and its copies on the node's other devices.
//
// Engine: RAII owner of one gpe_handle (one GP resident on one device).  QueryReplicas: one deep copy of a device model per OTHER
// visible device, made lazily by the first large query_batch() and kept while the handle it was cloned from and that handle's
// epoch (gpe_epoch) stand still.  The replicas belong to a handle, not to a model's value: they are never copied with the GP,
// and every path that changes which handle a GP holds goes through clear().
#ifndef LIMBO_MODEL_GP_REPLICAS_HPP
#define LIMBO_MODEL_GP_REPLICAS_HPP

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../../../gpe.h"

namespace limbo_amd {
    /// RAII owner of one engine handle (one GP resident on the device)
    class Engine {
    public:
        explicit Engine(int device) : _h(nullptr), _device(device) {}
        Engine(const Engine& o) : Engine(o, o._device) {}
        /// deep copy onto `device` (peer copy over xGMI when it differs from o's)
        Engine(const Engine& o, int device) : _h(nullptr), _device(device)
        {
            if (o._h)
                check(gpe_clone_to(o._h, _device, &_h), "gpe_clone_to");
        }
        Engine(Engine&& o) noexcept : _h(o._h), _device(o._device) { o._h = nullptr; }
        Engine& operator=(Engine&& o) noexcept
        {
            if (this != &o) {
                reset();
                _h = o._h;
                _device = o._device;
                o._h = nullptr;
            }
            return *this;
        }
        /// move the GP to another device of the node (no-op when it is there already)
        void set_device(int device)
        {
            if (device == _device)
                return;
            if (_h) {
                gpe_handle n = nullptr;
                check(gpe_clone_to(_h, device, &n), "gpe_clone_to");
                gpe_destroy(_h);
                _h = n;
            }
            _device = device;
        }
        Engine& operator=(const Engine& o)
        {
            if (this != &o) {
                reset();
                _device = o._device;
                if (o._h)
                    check(gpe_clone(o._h, &_h), "gpe_clone");
            }
            return *this;
        }
        ~Engine() { reset(); }
        void reset()
        {
            if (_h)
                gpe_destroy(_h);
            _h = nullptr;
        }
        gpe_handle get()
        {
            if (!_h)
                check(gpe_create(_device, &_h), "gpe_create");
            return _h;
        }
        gpe_handle peek() const { return _h; }
        int device() const { return _device; }
        /// negative status = API/HIP error: loud; positive = non-positive pivot: returned
        int check(int rc, const char* what) const
        {
            if (rc < 0)
                throw std::runtime_error(std::string("limbo_amd engine: ") + what + " failed (" + std::to_string(rc) + "): "
                    + (_h ? gpe_last_error(_h) : "no MI355X / libgpengine.so not usable"));
            return rc;
        }

    private:
        gpe_handle _h;
        int _device;
    };

    class QueryReplicas {
    public:
        QueryReplicas() = default;
        QueryReplicas(const QueryReplicas&) = delete;
        QueryReplicas& operator=(const QueryReplicas&) = delete;

        /// give the replicas back (device memory: one copy of the model on every other device)
        void clear()
        {
            std::lock_guard<std::mutex> lk(_mu);
            _engines.clear();
            _handle = nullptr;
            _epoch = 0;
        }
        /// how many devices the last batch was dealt over (1 + replicas alive)
        int devices() const
        {
            std::lock_guard<std::mutex> lk(_mu);
            return 1 + (int)_engines.size();
        }

        /// One GP's batch over ALL `ndev` visible devices (the reference's parallel query: multi_gp.hpp:191-195,
        /// tools/parallel.hpp:138-201 — TBB tasks over host cores there): device d answers a contiguous slice of the M points
        /// (Xq: row-major M x D) on its own replica of `own` (gpe_clone_to: a peer copy over xGMI, made once per state of the
        /// model and kept), one host thread per device, no collective: every slice lands in the caller's arrays (kta[point +
        /// M output], var[point]; either may be null).  Batched queries pick their kernels from N alone, so a point's answer
        /// does not depend on the slice it fell into: the result is bitwise the one-device answer.
        void query(Engine& own, int ndev, const double* Xq, int64_t M, int D, int P, double* kta, double* var)
        {
            std::lock_guard<std::mutex> lk(_mu);
            uint64_t ep = 0;
            own.check(gpe_epoch(own.get(), &ep), "gpe_epoch");
            if ((int)_engines.size() != ndev - 1 || _handle != own.peek() || _epoch != ep) {
                _engines.clear();
                _engines.reserve((size_t)(ndev - 1));
                for (int d = 0; d < ndev; ++d)
                    if (d != own.device())
                        _engines.emplace_back(own, d);
                _handle = own.peek();
                _epoch = ep;
            }
            auto lo_of = [&](int k) { return (int64_t)k * (M / ndev) + std::min<int64_t>(k, M % ndev); }; // (parallel.py: row_slice)
            std::vector<std::string> errs((size_t)ndev);
            auto work = [&](int k, Engine* e) {
                try {
                    const int64_t lo = lo_of(k), m = lo_of(k + 1) - lo;
                    if (m <= 0)
                        return;
                    if (P == 1 || !kta) {
                        e->check(gpe_query_batch(e->get(), Xq + lo * D, m, kta ? kta + lo : nullptr, var ? var + lo : nullptr), "gpe_query_batch");
                        return;
                    }
                    std::vector<double> kl((size_t)(m * P)); // kta is [point + M output]: a slice is not contiguous in it
                    e->check(gpe_query_batch(e->get(), Xq + lo * D, m, kl.data(), var ? var + lo : nullptr), "gpe_query_batch");
                    for (int p = 0; p < P; ++p)
                        std::copy(kl.begin() + (size_t)(m * p), kl.begin() + (size_t)(m * (p + 1)), kta + lo + M * p);
                }
                catch (const std::exception& ex) {
                    errs[(size_t)k] = ex.what();
                }
            };
            {
                struct Joined { // (a thread that cannot be started throws out of emplace_back: the ones running are joined first)
                    std::vector<std::thread> th;
                    ~Joined()
                    {
                        for (auto& t : th)
                            t.join();
                    }
                } workers;
                workers.th.reserve(_engines.size());
                int slot = 1; // slice 0 is the model's own device (this thread), slices 1.. the replicas in device order
                for (auto& r : _engines)
                    workers.th.emplace_back(work, slot++, &r);
                work(0, &own);
            }
            for (auto& e : errs)
                if (!e.empty())
                    throw std::runtime_error(e);
        }

    private:
        std::vector<Engine> _engines;
        gpe_handle _handle = nullptr; // the key: the handle the replicas were cloned from ...
        uint64_t _epoch = 0;          // ... and its epoch then
        mutable std::mutex _mu;
    };
} // namespace limbo_amd

#endif
