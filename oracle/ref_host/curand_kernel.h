/*
 * curand_kernel.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Host stand-in for the one header the reference's kernel file includes.  With this directory first on
 * the include path (-Ioracle/ref_host) g++ compiles that file as plain C++ and every kernel and device
 * function becomes a C symbol.  Written from CUDA's public programming model, not from the reference:
 * it declares no kernel, no prototype and no struct of the reference's.
 *
 * Execution model (see ref_launch.cpp): one OS thread per CUDA thread of a block, the blocks of a grid
 * one after another, __syncthreads() a real barrier among the block's threads.  __shared__ variables
 * become function-local statics, which all threads of the running block share; the next block starts only
 * after every thread of the previous one has returned.
 *
 * What this pins and what it does not: the semantics of the program text as written, evaluated with
 * glibc's powf/expf/logf/log/sqrt and without fused multiply-add (-ffp-contract=off).  It does not pin
 * nvcc's FMA contraction or CUDA's libm (a few ulp), exactly as graal_oracle.c does not.
 *
 * ---------------------------------------------------------------------------------------------------
 * Math calls of the kernels under test, and the overload CUDA's headers select for them.  CUDA puts a
 * float overload of every <math.h> function into the global namespace, so a call whose arguments are all
 * float (or float and int for pow) runs in single precision; host C++ with only <math.h>'s C prototypes
 * would silently promote to double.  The overloads below restore CUDA's choice.  "line" is the line of
 * kernels3.cu; the last column is what graal_oracle.c calls at the same place.
 *
 *  line  function                     call                              argument types     CUDA picks   oracle
 *  ----  ---------------------------  --------------------------------  -----------------  -----------  ----------
 *    84  factorial                    floor(n)                          float              floorf       floorf
 *    90  factorial                    powf(n,n)                         float,float        powf         powf
 *    90  factorial                    exp(-n)                           float              expf         expf
 *    90  factorial                    sqrtf(2 * M_PI * n)               double -> float    sqrtf        sqrtf((float)..)
 *   126  rippe_contacts               pow(s, p.slope)                   float,float        powf         powf
 *   126  rippe_contacts               pow(s*p.lm/p.kuhn, 2.0f)          float,float        powf         powf
 *   126  rippe_contacts               exp((p.d-2)/(.. + p.d))           float              expf         expf
 *   128  rippe_contacts               max(result, p.v_inter)            float,float        fmaxf        fmaxf
 *   156  rippe_contacts_circ          powf x3, expf                     float              as written   as written
 *   158  rippe_contacts_circ          powf x3, expf                     float              as written   as written
 *   161  rippe_contacts_circ          max(result, p.v_inter)            float,float        fmaxf        fmaxf
 *   199  evaluate_likelihood_double   log(ex), log(ob)                  double             log          log
 *   199  evaluate_likelihood_double   log(sqrt(ob * 2.0 * M_PI))        double             log, sqrt    log, sqrt
 *   202  evaluate_likelihood_double   log((double) factorial(..))       double             log          log
 *   217  lin_2_2dpos                  sqrt((float) 1 + 8 * (i - 1))     float (float+int)  sqrtf        (loops, no sqrt)
 *   221  lin_2_2dpos                  min / max (x - 1, y - 1)          int,int            int          --
 *   230  conv_plan_pos_2_lin          min / max (x, y)                  int,int            int          pix_index
 *  3064  evaluate_likelihood          fabsf(list_s_fj[j]-list_s_fi[i])  float              fabsf        fabsf
 *  3550  sub_compute_likelihood       fabsf(..)                         float              fabsf        fabsf
 *  3360+ sub_compute_likelihood       min / max (tmp_id_data_fi, _fj)   int,int            int          lo / hi
 *
 * Not under test but compiled: evaluate_likelihood_float (logf, sqrtf as written), gen_rand_mat line 72
 * max(float, 0.000001) -> CUDA's mixed overload max(float,double) returns double.
 * ---------------------------------------------------------------------------------------------------
 */
#ifndef GRAAL_REF_HOST_CURAND_KERNEL_H
#define GRAAL_REF_HOST_CURAND_KERNEL_H

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>

/* ---- qualifiers ------------------------------------------------------------------------------------ */
#define __global__
#define __device__
#define __host__
#define __constant__ static
#define __shared__ static
#define __forceinline__ inline
/* __restrict is a g++ keyword already */

/* ---- vector types ---------------------------------------------------------------------------------- */
struct uint3 { unsigned int x, y, z; };
struct dim3 { unsigned int x, y, z; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct alignas(16) int4 { int x, y, z, w; };
struct alignas(8) float2 { float x, y; };
struct float3 { float x, y, z; };
struct alignas(16) float4 { float x, y, z, w; };
struct uchar4 { unsigned char x, y, z, w; };
static inline int2 make_int2(int x, int y) { int2 v = {x, y}; return v; }
static inline int3 make_int3(int x, int y, int z) { int3 v = {x, y, z}; return v; }
static inline int4 make_int4(int x, int y, int z, int w) { int4 v = {x, y, z, w}; return v; }
static inline float2 make_float2(float x, float y) { float2 v = {x, y}; return v; }
static inline float3 make_float3(float x, float y, float z) { float3 v = {x, y, z}; return v; }
static inline float4 make_float4(float x, float y, float z, float w) { float4 v = {x, y, z, w}; return v; }

/* ---- built-in variables: per OS thread, set by the launcher ----------------------------------------- */
inline thread_local uint3 threadIdx = {0, 0, 0};
inline thread_local uint3 blockIdx = {0, 0, 0};
inline dim3 blockDim = {1, 1, 1};
inline dim3 gridDim = {1, 1, 1};

/* dynamic shared memory of the running launch (shared_bytes, zero padded); the one patched line of the
 * generated kernel copy points the kernel's dynamic array here */
inline void *ref_host_dynamic_shared = nullptr;

/* block barrier, provided by the launcher */
void ref_host_syncthreads();
#define __syncthreads() ref_host_syncthreads()

/* ---- atomics ---------------------------------------------------------------------------------------- */
inline std::mutex ref_host_atomic_mutex;
template <typename T> static inline T ref_host_atomic_add(T *address, T val)
{
    std::lock_guard<std::mutex> g(ref_host_atomic_mutex);
    T old = *address;
    *address = old + val;
    return old;
}
static inline double atomicAdd(double *a, double v) { return ref_host_atomic_add(a, v); }
static inline float atomicAdd(float *a, float v) { return ref_host_atomic_add(a, v); }
static inline int atomicAdd(int *a, int v) { return ref_host_atomic_add(a, v); }
static inline unsigned int atomicAdd(unsigned int *a, unsigned int v) { return ref_host_atomic_add(a, v); }

/* ---- CUDA's math overload set in the global namespace ------------------------------------------------ */
static inline float pow(float a, float b) { return powf(a, b); }
static inline float pow(float a, int b) { return powf(a, (float)b); }
static inline float exp(float a) { return expf(a); }
static inline float log(float a) { return logf(a); }
static inline float sqrt(float a) { return sqrtf(a); }
static inline float floor(float a) { return floorf(a); }
static inline float ceil(float a) { return ceilf(a); }
static inline float abs(float a) { return fabsf(a); }
static inline float fabs(float a) { return fabsf(a); }

/* CUDA's type-conversion intrinsics with their default rounding: int2float rounds to nearest even, as the
 * C cast does; float2int truncates.  evaluate_likelihood and sub_compute_likelihood use int2float for
 * l_cont_bp (lines 2954, 3448) and for the product of two RF counts (lines 3187, 3671). */
static inline float int2float(int a) { return (float)a; }
static inline int float2int(float a) { return (int)a; }
static inline float __int2float_rn(int a) { return (float)a; }
static inline int __float2int_rz(float a) { return (int)a; }
static inline int __float2int_rd(float a) { return (int)floorf(a); }

static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
static inline unsigned int min(unsigned int a, unsigned int b) { return a < b ? a : b; }
static inline unsigned int max(unsigned int a, unsigned int b) { return a > b ? a : b; }
static inline unsigned int min(int a, unsigned int b) { return min((unsigned int)a, b); }
static inline unsigned int max(int a, unsigned int b) { return max((unsigned int)a, b); }
static inline unsigned int min(unsigned int a, int b) { return min(a, (unsigned int)b); }
static inline unsigned int max(unsigned int a, int b) { return max(a, (unsigned int)b); }
static inline float min(float a, float b) { return fminf(a, b); }
static inline float max(float a, float b) { return fmaxf(a, b); }
static inline double min(double a, double b) { return fmin(a, b); }
static inline double max(double a, double b) { return fmax(a, b); }
static inline double min(float a, double b) { return fmin((double)a, b); }
static inline double max(float a, double b) { return fmax((double)a, b); }
static inline double min(double a, float b) { return fmin(a, (double)b); }
static inline double max(double a, float b) { return fmax(a, (double)b); }

/* ---- inert stubs: textures and curand.  No kernel under test touches them; a call aborts. ------------- */
[[noreturn]] static inline void ref_host_unsupported(const char *what)
{
    std::fprintf(stderr, "ref_host: %s is a stub; the calling kernel is not under test\n", what);
    std::abort();
}

enum cudaTextureReadMode { cudaReadModeElementType = 0, cudaReadModeNormalizedFloat = 1 };
template <typename T, int Dim = 1, int Mode = cudaReadModeElementType> struct texture { };
template <typename T, int Dim, int Mode> static inline T tex2D(texture<T, Dim, Mode>, float, float)
{
    ref_host_unsupported("tex2D");
}
template <typename T, int Dim, int Mode> static inline T tex1Dfetch(texture<T, Dim, Mode>, int)
{
    ref_host_unsupported("tex1Dfetch");
}

struct curandState { unsigned long long opaque[6]; };
typedef curandState curandState_t;
static inline void curand_init(unsigned long long, unsigned long long, unsigned long long, curandState *)
{
    ref_host_unsupported("curand_init");
}
static inline unsigned int curand(curandState *) { ref_host_unsupported("curand"); }
static inline unsigned int curand_poisson(curandState *, double) { ref_host_unsupported("curand_poisson"); }
static inline float curand_uniform(curandState *) { ref_host_unsupported("curand_uniform"); }
static inline float curand_normal(curandState *) { ref_host_unsupported("curand_normal"); }

#endif
