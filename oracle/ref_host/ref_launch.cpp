/*
 * ref_launch.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Host launcher for the reference's kernel file.  The file is included by a path given at compile time
 * (-DREF_KERNELS="\"...\""); nothing of it is restated here: every entry point takes its kernel's
 * arguments the way cuLaunchKernel does, as an array of pointers to the argument values, and a template
 * reads their types off the kernel's own declaration.
 *
 *   ref_launch_<kernel>(grid, block, shared_bytes, void **args)   run a grid
 *   ref_nargs_<kernel>(int *sizes)                                number of arguments, sizeof of each
 *   ref_call_<function>(void *ret, void **args)                   one call of a device function
 *
 * Execution model: a pool of OS threads, one per CUDA thread of a block.  The blocks of a grid run one
 * after another; inside a block the threads run concurrently and __syncthreads() is a barrier among
 * them, so both patterns of the file are honoured: "thread 0 fills block-shared scalars, barrier, all
 * read" and "all write res[threadIdx.x], barrier, thread 0 sums".  A second barrier closes each block, so
 * the statics that stand for __shared__ variables are never overwritten while a block still reads them.
 * Grids are one-dimensional (x only), as every launch of the kernels under test is.
 */
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include <curand_kernel.h>

#ifndef REF_KERNELS
#error "compile with -DREF_KERNELS=\"<path of the generated kernel copy>\""
#endif
#include REF_KERNELS

namespace {

/* reusable barrier for a fixed number of threads, counted by generation.  The threads of a block are all runnable for the
 * length of a launch, so a waiter spins a little and then yields its time slice instead of sleeping: with more threads than
 * cores a sleeping barrier costs a wake-up per thread per barrier, which dominates kernels this small. */
class Barrier {
  public:
    void reset(int n) { n_ = n; count_.store(0); }
    void wait()
    {
        const unsigned gen = gen_.load(std::memory_order_acquire);
        if (count_.fetch_add(1, std::memory_order_acq_rel) + 1 == n_) {
            count_.store(0, std::memory_order_relaxed);
            gen_.fetch_add(1, std::memory_order_release); /* publishes the reset count and everything before the barrier */
        } else {
            for (int spins = 0; gen_.load(std::memory_order_acquire) == gen; spins++)
                if (spins >= 32) std::this_thread::yield();
        }
    }

  private:
    std::atomic<int> count_{0};
    std::atomic<unsigned> gen_{0};
    int n_ = 1;
};

Barrier g_block_barrier;

/* persistent workers: worker t plays threadIdx.x == t of every block of the current launch */
class Pool {
  public:
    ~Pool()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            quit_ = true;
        }
        cv_.notify_all();
        for (auto &t : workers_) t.join();
    }

    void run(int grid, int block, const std::function<void()> &kernel)
    {
        std::unique_lock<std::mutex> lk(m_);
        while ((int)workers_.size() < block) {
            const int tid = (int)workers_.size();
            const unsigned seen = job_; /* born before the job is posted: takes it too */
            workers_.emplace_back([this, tid, seen] { loop(tid, seen); });
        }
        grid_ = grid; block_ = block; kernel_ = &kernel; done_ = 0;
        ++job_;
        cv_.notify_all();
        done_cv_.wait(lk, [&] { return done_ == block_; });
        kernel_ = nullptr;
    }

  private:
    void loop(int tid, unsigned seen)
    {
        for (;;) {
            int grid, block;
            const std::function<void()> *kernel;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return quit_ || job_ != seen; });
                if (quit_) return;
                seen = job_;
                grid = grid_; block = block_; kernel = kernel_;
            }
            if (tid >= block) continue;
            threadIdx.x = (unsigned)tid; threadIdx.y = 0; threadIdx.z = 0;
            for (int b = 0; b < grid; b++) {
                blockIdx.x = (unsigned)b; blockIdx.y = 0; blockIdx.z = 0;
                (*kernel)();
                g_block_barrier.wait(); /* end of block: nobody starts block b+1 before all left block b */
            }
            {
                std::lock_guard<std::mutex> lk(m_);
                if (++done_ == block) done_cv_.notify_all();
            }
        }
    }

    std::mutex m_;
    std::condition_variable cv_, done_cv_;
    std::vector<std::thread> workers_;
    const std::function<void()> *kernel_ = nullptr;
    int grid_ = 0, block_ = 0, done_ = 0;
    unsigned job_ = 0;
    bool quit_ = false;
};

Pool &pool()
{
    static Pool *p = new Pool; /* never destroyed: workers must not be joined from an exit handler */
    return *p;
}

std::mutex g_launch_mutex; /* one launch at a time, whoever calls */

void run_grid(int grid, int block, size_t shared_bytes, const std::function<void()> &kernel)
{
    std::lock_guard<std::mutex> lk(g_launch_mutex);
    /* dynamic shared memory: shared_bytes, plus a zeroed pad so that a kernel reading a little past its
     * array does not leave the buffer */
    std::vector<double> shared((shared_bytes + sizeof(double) - 1) / sizeof(double) + 64, 0.0);
    ref_host_dynamic_shared = shared.data();
    gridDim.x = (unsigned)grid; gridDim.y = 1; gridDim.z = 1;
    blockDim.x = (unsigned)block; blockDim.y = 1; blockDim.z = 1;
    g_block_barrier.reset(block);
    pool().run(grid, block, kernel);
    ref_host_dynamic_shared = nullptr;
}

template <typename T> using arg_t = std::remove_cv_t<std::remove_reference_t<T>>;

template <typename... A, size_t... I>
void launch_impl(void (*k)(A...), int grid, int block, size_t shm, void **args, std::index_sequence<I...>)
{
    run_grid(grid, block, shm, [&] { k(*static_cast<arg_t<A> *>(args[I])...); });
}

template <typename... A> void launch(void (*k)(A...), int grid, int block, size_t shm, void **args)
{
    launch_impl(k, grid, block, shm, args, std::index_sequence_for<A...>{});
}

template <typename... A> int nargs(void (*)(A...), int *sizes)
{
    const int s[] = {(int)sizeof(arg_t<A>)..., 0};
    if (sizes)
        for (size_t i = 0; i < sizeof...(A); i++) sizes[i] = s[i];
    return (int)sizeof...(A);
}

template <typename R, typename... A, size_t... I>
void call_impl(R (*f)(A...), void *ret, void **args, std::index_sequence<I...>)
{
    *static_cast<R *>(ret) = f(*static_cast<arg_t<A> *>(args[I])...);
}

template <typename R, typename... A> void call(R (*f)(A...), void *ret, void **args)
{
    call_impl(f, ret, args, std::index_sequence_for<A...>{});
}

template <typename R, typename... A> int nargs(R (*)(A...), int *sizes, int *ret_size)
{
    const int s[] = {(int)sizeof(arg_t<A>)..., 0};
    if (sizes)
        for (size_t i = 0; i < sizeof...(A); i++) sizes[i] = s[i];
    if (ret_size) *ret_size = (int)sizeof(R);
    return (int)sizeof...(A);
}

}  // namespace

void ref_host_syncthreads() { g_block_barrier.wait(); }

#define REF_KERNEL(name)                                                                        \
    extern "C" void ref_launch_##name(int grid, int block, size_t shared_bytes, void **args)    \
    {                                                                                           \
        launch(name, grid, block, shared_bytes, args);                                          \
    }                                                                                           \
    extern "C" int ref_nargs_##name(int *sizes) { return nargs(name, sizes); }

#define REF_FUNCTION(name)                                                                      \
    extern "C" void ref_call_##name(void *ret, void **args) { call(name, ret, args); }          \
    extern "C" int ref_nargs_##name(int *sizes, int *ret_size) { return nargs(name, sizes, ret_size); }

/* the kernels under test, by name only */
REF_KERNEL(copy_struct)
REF_KERNEL(simple_copy)
REF_KERNEL(flip_frag)
REF_KERNEL(swap_activity_frag)
REF_KERNEL(pop_out_frag)
REF_KERNEL(pop_in_frag_1)
REF_KERNEL(pop_in_frag_2)
REF_KERNEL(pop_in_frag_3)
REF_KERNEL(pop_in_frag_4)
REF_KERNEL(split_contig)
REF_KERNEL(paste_contigs)
REF_KERNEL(fill_sub_index_fA)
REF_KERNEL(fill_sub_index_fB)
REF_KERNEL(evaluate_likelihood)
REF_KERNEL(sub_compute_likelihood)

REF_FUNCTION(factorial)
REF_FUNCTION(rippe_contacts)
REF_FUNCTION(rippe_contacts_circ)
REF_FUNCTION(evaluate_likelihood_double)
