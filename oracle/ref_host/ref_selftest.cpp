/*
 * ref_selftest.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Stand-alone program (its own main, no Python): runs every kernel under test once through the launcher on the
 * likelihood toy of SURVEY Appendix E (6 bins of 3 sub-fragments, two contigs of 3 bins, observations from the toy's
 * linear congruential generator) and prints what they give.  Buffers have exactly the size the kernels are entitled
 * to, so a build with the host sanitizers (make -C oracle _ref/ref_selftest SAN=1) reports any read or write of the
 * reference's text outside them -- with one exception, which is what that build found: paste_contigs and
 * pop_in_frag_1..4 load entry [global thread index] of every field of the SOURCE layout before they compare the index
 * with n_frags (kernels3.cu:1841-1853, 644 ff.), so the fragment arrays are padded to one entry per launched thread
 * (PAD), as oracle/ref_kernels.py pads them.  Built and run by hand; not part of build() or of the test-suite.
 */
#include "ref_launch.cpp"

#include <cstdio>

namespace {

constexpr int N = 6, NSUB = 3, S = N * NSUB, GRID = 2, BLOCK = 32, PAD = GRID * BLOCK;

struct Layout {
    std::vector<int> f[14];
    frag dev;
    Layout()
    {
        for (auto &v : f) v.assign(PAD, 0);
        int **slot = reinterpret_cast<int **>(&dev);
        for (int k = 0; k < 14; k++) slot[k] = f[k].data();
    }
};

void toy(Layout &l)
{
    for (int i = 0; i < N; i++) {
        const int c = i / 3, k = i % 3;
        l.dev.pos[i] = k; l.dev.id_c[i] = c; l.dev.start_bp[i] = 3000 * k; l.dev.len_bp[i] = 3000;
        l.dev.circ[i] = 0; l.dev.id[i] = i; l.dev.prev[i] = k ? i - 1 : -1; l.dev.next[i] = k < 2 ? i + 1 : -1;
        l.dev.l_cont[i] = 3; l.dev.l_cont_bp[i] = 9000; l.dev.ori[i] = 1; l.dev.rep[i] = 0; l.dev.activ[i] = 1;
        l.dev.id_d[i] = i;
    }
}

void show(const char *what, const Layout &l)
{
    std::printf("%-22s", what);
    for (int i = 0; i < N; i++)
        std::printf(" [c%d p%d s%d o%d <%d >%d n%d]", l.dev.id_c[i], l.dev.pos[i], l.dev.start_bp[i], l.dev.ori[i],
                    l.dev.prev[i], l.dev.next[i], l.dev.l_cont[i]);
    std::printf("\n");
}

template <typename... T> void go(void (*entry)(int, int, size_t, void **), size_t shm, T... a)
{
    void *args[] = {static_cast<void *>(&a)...};
    entry(GRID, BLOCK, shm, args);
}

}  // namespace

int main()
{
    Layout cur, out, tmp, tmp2;
    toy(cur);
    frag *pc = &cur.dev, *po = &out.dev, *pt = &tmp.dev, *pt2 = &tmp2.dev;
    std::vector<int> ids(N, 0);
    int *pids = ids.data();
    show("toy", cur);

    go(ref_launch_simple_copy, 0, po, pc, N); show("simple_copy", out);
    go(ref_launch_copy_struct, 0, po, pc, pids, N); show("copy_struct", out);
    go(ref_launch_flip_frag, 0, po, pc, 1, N); show("flip_frag 1", out);
    go(ref_launch_pop_out_frag, 0, pt, pc, pids, 1, 1, N); show("pop_out_frag 1", tmp);
    go(ref_launch_swap_activity_frag, 0, po, pt, 1, 2, N); show("swap_activity 1", out);
    go(ref_launch_pop_in_frag_1, 0, po, pt, 1, 4, 2, 1, N); show("pop_in_1 1 @ 4", out);
    go(ref_launch_pop_in_frag_2, 0, po, pt, 1, 4, 2, -1, N); show("pop_in_2 1 @ 4", out);
    go(ref_launch_pop_in_frag_3, 0, po, pt, 1, 4, 2, 1, N); show("pop_in_3 1 @ 4", out);
    go(ref_launch_pop_in_frag_4, 0, po, pt, 1, 4, 2, -1, N); show("pop_in_4 1 @ 4", out);
    go(ref_launch_split_contig, 0, pt, pc, pids, 1, 0, 1, N); show("split 1 downstream", tmp);
    go(ref_launch_split_contig, 0, pt2, pt, pids, 4, 1, 2, N); show("split 4 upstream", tmp2);
    toy(out);
    go(ref_launch_paste_contigs, 0, po, pt2, 1, 4, 3, N); show("paste 1 + 4", out);
    toy(out);
    go(ref_launch_paste_contigs, 0, po, pc, 1, 1, 1, N); show("paste 1 + 1 (stale)", out);

    std::vector<int> sub_index(N, -1);
    int *psub = sub_index.data();
    go(ref_launch_fill_sub_index_fA, 0, pc, psub, 0, N);
    go(ref_launch_fill_sub_index_fB, 0, pc, psub, 1, 3, N);
    std::printf("%-22s", "fill_sub_index");
    for (int v : sub_index) std::printf(" %d", v);
    std::printf("\n");

    /* likelihood data of the toy */
    std::vector<float> obs((size_t)S * S, 0.0f);
    unsigned long long seed = 1;
    for (int i = 0; i < S; i++)
        for (int j = i + 1; j < S; j++) {
            seed = (seed * 1664525ull + 1013904223ull) % (1ull << 32);
            const unsigned m = (i / 9 == j / 9) ? 20u : 3u;
            obs[(size_t)i * S + j] = obs[(size_t)j * S + i] = (float)((seed >> 24) % m);
        }
    std::vector<int4> sub_id(N);
    std::vector<float3> sub_len(N);
    std::vector<int3> sub_accu(N);
    std::vector<int2> disp(N);
    std::vector<int> coll(N);
    for (int i = 0; i < N; i++) {
        sub_id[i] = make_int4(3 * i, 3 * i + 1, 3 * i + 2, 3);
        sub_len[i] = make_float3(1.0f, 1.0f, 1.0f);
        sub_accu[i] = make_int3(1, 1, 1);
        disp[i] = make_int2(i, i + 1);
        coll[i] = i;
    }
    param_simu p;
    p.kuhn = 1.0f; p.lm = 9.6f; p.c1 = (float)(0.53 * std::pow(9.6, -1.5)); p.slope = -1.5f; p.d = 3.0f;
    p.d_max = 500.0f; p.fact = 50.0f; p.v_inter = 0.05f;
    param_simu *pp = &p;
    const int n_up = N * (N - 1) / 2, n_pix = n_up + N;
    std::vector<double> pix(n_pix, 0.0);
    const float *pobs = obs.data();
    int *pcoll = coll.data();
    int2 *pdisp = disp.data();
    int4 *pid = sub_id.data();
    float3 *plen = sub_len.data();
    int3 *paccu = sub_accu.data();
    double *ppix = pix.data();
    go(ref_launch_evaluate_likelihood, 0, pobs, pc, pcoll, pdisp, pid, pid, plen, paccu, ppix, pp, n_up, n_pix, N, S, 1.0f);
    double full = 0.0;
    for (double v : pix) full += v;
    std::printf("evaluate_likelihood    %.12f\n", full);

    go(ref_launch_pop_out_frag, 0, pt, pc, pids, 1, 1, N);
    std::vector<int> no_rep = {0, 1, 2}, rep = {-1}, uniq = {0, 1, 2, 3, 4, 5};
    int *pno = no_rep.data(), *prep = rep.data(), *puniq = uniq.data();
    double delta = 0.0, *pdelta = &delta;
    go(ref_launch_sub_compute_likelihood, (size_t)BLOCK * 8, pobs, pt, pno, prep, puniq, pcoll, pdisp, pid, plen, paccu, pdelta,
       ppix, pp, 3, 3, 3, 3, 6, 0, S, N, 1.0f);
    std::printf("sub_compute_likelihood %.12f\n", delta);

    float s = 2.0f, s_tot = 40.0f, r = 0.0f, n12 = 12.0f;
    double ex = 2.0, ob = 3.0, l = 0.0;
    void *a1[] = {&s, &p};
    ref_call_rippe_contacts(&r, a1); std::printf("rippe_contacts(2)      %.9g\n", r);
    void *a2[] = {&s, &s_tot, &p};
    ref_call_rippe_contacts_circ(&r, a2); std::printf("rippe_contacts_circ    %.9g\n", r);
    void *a3[] = {&ex, &ob};
    ref_call_evaluate_likelihood_double(&l, a3); std::printf("evaluate_likelihood_d  %.12f\n", l);
    void *a4[] = {&n12};
    ref_call_factorial(&r, a4); std::printf("factorial(12)          %.9g\n", r);
    return 0;
}
