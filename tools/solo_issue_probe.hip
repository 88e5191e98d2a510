// Price list for a lone wave on gfx950: what one instruction of each kind the solo K4 step is made of costs a wave that has its SIMD to
// itself (the net waves of mh_kernel_solo run one per SIMD and pay for every instruction they issue).
// Developer tool, not part of the library:
//   hipcc --offload-arch=gfx950 -O3 tools/solo_issue_probe.hip -o tools/bin/solo_issue_probe && tools/bin/solo_issue_probe > profiles/r10/solo_issue_costs.txt
//
// One workgroup of four waves, one per SIMD.  Every wave runs, kind by kind, a loop of ITERS passes over BODY instructions of that one
// kind between two s_memtime reads (the clock of the NNEST_STAMP builds): first with independent operands (eight rotating
// destinations), then with each instruction reading what the one before it wrote.  An empty loop of the same shape is measured too and
// subtracted.  Second pass: the same with a fifth wave that runs a plain v_fma_f32 stream for as long as the others measure -- it
// lands beside one of them, which then shares its SIMD the way net wave 0 shares SIMD 0 with the noise wave.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>

#define ITERS 32
#define BODY 64   // 8 x the 8-way .irp below
#define XSTR(x) #x
#define STR(x) XSTR(x)

// v10..v25: destinations (eight registers or eight aligned pairs), v30..v37: sources nobody writes, v40: the lane's LDS address,
// s[20:21]: a lane mask, s22..s29: scalar destinations.
#define CLOBBERS "v10", "v11", "v12", "v13", "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", \
                 "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v40", "s20", "s21", "s22", "s23", "s24", "s25", "s26", "s27", "s28", "s29", "vcc", "scc", "memory"

// \r runs over the eight destination registers (REGS1) or the low registers of the eight destination pairs (REGS2)
#define REGS1 "10,11,12,13,14,15,16,17"
#define REGS2 "10,12,14,16,18,20,22,24"
#define SREGS "22,23,24,25,26,27,28,29"

#define STREAM(slot, regs, body)                                                                                        \
    do {                                                                                                                \
        unsigned long long t0_, t1_;                                                                                    \
        unsigned cnt_;                                                                                                  \
        asm volatile(                                                                                                   \
            "v_mov_b32 v30, 1.0\n v_mov_b32 v31, 0.5\n v_mov_b32 v32, 2.0\n v_mov_b32 v33, 0.5\n"                       \
            "v_mov_b32 v34, 1.0\n v_mov_b32 v35, 0.5\n v_mov_b32 v36, 2.0\n v_mov_b32 v37, 0x1f8\n"                     \
            ".irp r,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25\n v_mov_b32 v\\r, 1.0\n .endr\n"                    \
            "v_mov_b32 v40, %3\n s_mov_b64 s[20:21], 0x55555555\n s_mov_b32 s22, 0\n s_mov_b32 s23, 0\n"                \
            "s_movk_i32 %2, " STR(ITERS) "\n s_nop 7\n"                                                                 \
            "s_memtime %0\n s_waitcnt lgkmcnt(0)\n"                                                                     \
            "1:\n .rept 8\n .irp r," regs "\n" body "\n .endr\n .endr\n"                                                \
            "s_sub_u32 %2, %2, 1\n s_cmp_lg_u32 %2, 0\n s_cbranch_scc1 1b\n"                                            \
            "s_memtime %1\n s_waitcnt lgkmcnt(0)\n"                                                                     \
            : "=&s"(t0_), "=&s"(t1_), "=&s"(cnt_) : "v"(lds_addr) : CLOBBERS);                                          \
        if (lane == 0) cyc[((pass * NKIND + (slot)) * 5) + wave] = t1_ - t0_;                                            \
    } while (0)

struct Kind { const char *name; int per;   // instructions per .irp step (a pair counts as its two)
              const char *note; };
static const Kind KINDS[] = {
    {"(empty loop: 2 SALU + branch per pass)", 0, ""},
    {"v_fma_f32                         indep", 1, ""},
    {"v_fma_f32                         dep", 1, ""},
    {"v_mul_f32                         indep", 1, ""},
    {"v_mov_b32                         indep", 1, ""},
    {"v_fmac_f32_dpp row_ror            indep", 1, "eight accumulators"},
    {"v_fmac_f32_dpp row_ror            dep", 1, "one accumulator, as a chain of the coupling blocks"},
    {"v_mov_b32_dpp row_ror             indep", 1, ""},
    {"v_mov_b32_dpp row_ror + s_nop 1   dep", 2, "the pair; DPP reads what the move before it wrote"},
    {"v_add_f32_dpp row_ror             indep", 1, ""},
    {"v_add_f32_dpp row_ror             dep", 1, "through the plain operand"},
    {"v_pk_mul_f32                      indep", 1, ""},
    {"v_pk_mul_f32                      dep", 1, ""},
    {"v_pk_add_f32                      indep", 1, ""},
    {"v_pk_add_f32                      dep", 1, ""},
    {"v_pk_fma_f32                      indep", 1, ""},
    {"v_pk_fma_f32                      dep", 1, ""},
    {"v_exp_f32                         indep", 1, ""},
    {"v_exp_f32                         dep", 1, ""},
    {"v_rcp_f32                         indep", 1, ""},
    {"v_rcp_f32                         dep", 1, ""},
    {"v_exp_f32 + s_nop 0 + v_add_f32   dep", 3, "the triple; a plain VALU reads the transcendental"},
    {"v_permlane16_swap_b32             indep", 1, "no pad: nobody reads the pair for eight instructions"},
    {"v_permlane16_swap_b32 + s_nop 1   dep", 2, "the pair"},
    {"v_permlane32_swap_b32             indep", 1, "no pad"},
    {"v_permlane32_swap_b32 + s_nop 1   dep", 2, "the pair"},
    {"v_bfi_b32                         indep", 1, ""},
    {"v_bfi_b32                         dep", 1, ""},
    {"v_cndmask_b32_e64 (SGPR pair)     indep", 1, ""},
    {"v_cndmask_b32_e64 (SGPR pair)     dep", 1, ""},
    {"v_cvt_f64_f32                     indep", 1, ""},
    {"v_cvt_f64_f32                     dep", 1, ""},
    {"v_cvt_f32_f64                     indep", 1, ""},
    {"v_fma_f64                         indep", 1, ""},
    {"v_fma_f64                         dep", 1, ""},
    {"v_cmp_gt_f64 vcc                  indep", 1, ""},
    {"v_cmp_gt_f64 vcc + v_cndmask vcc  dep", 2, "the pair; the compare reads the select's result"},
    {"v_cmp_gt_f32 vcc                  indep", 1, ""},
    {"v_cmp_class_f32 vcc               indep", 1, ""},
    {"v_cmp_class_f32 vcc + v_cndmask   dep", 2, "the pair"},
    {"v_max3_f32 |a|,|b|,|c|            indep", 1, ""},
    {"v_max3_f32 |a|,|b|,|c|            dep", 1, ""},
    {"v_add3_u32                        indep", 1, ""},
    {"v_add3_u32                        dep", 1, ""},
    {"s_nop 0", 1, ""},
    {"s_nop 1", 1, "one instruction, two wait states"},
    {"s_add_u32                         indep", 1, ""},
    {"s_add_u32                         dep", 1, ""},
    {"s_and_b64                         indep", 1, ""},
    {"ds_read_b128 + s_waitcnt lgkmcnt(0)", 2, "the pair"},
    {"4 x ds_read_b128 + s_waitcnt      ", 5, "the five"},
    {"v_fma_f32, v_fma_f32 (two plain)  indep", 2, "the two a v_pk_fma_f32 replaces"},
    {"v_mul_f32, v_mul_f32 (two plain)  dep", 2, "two chains side by side, what one dependent v_pk_mul_f32 carries"},
};
#define NKIND ((int)(sizeof(KINDS) / sizeof(KINDS[0])))
#define NKIND_MAX 64

__global__ void __launch_bounds__(320) probe_kernel(unsigned long long *cyc, unsigned *simd, float *sink, int pass) {
    __shared__ float lds[1024];        // 16 bytes per lane of four waves
    __shared__ volatile int done;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    lds[threadIdx.x & 1023] = 1.0f;
    lds[(threadIdx.x + 320) & 1023] = 1.0f;
    lds[(threadIdx.x + 640) & 1023] = 1.0f;
    lds[(threadIdx.x + 960) & 1023] = 1.0f;
    if (threadIdx.x == 0) done = 0;
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID, 4, 2)" : "=s"(id));
    if (lane == 0) simd[pass * 5 + wave] = id;
    __syncthreads();
    if (wave == 4) {
        // the neighbour: a plain VALU stream until the four others are through
        float a = 1.0f + lane, acc = 0.f;
        while (done < 4) {
            asm volatile(".rept 64\n v_fma_f32 %0, %1, %1, %0\n .endr" : "+v"(acc) : "v"(a));
        }
        sink[threadIdx.x] = acc;
        return;
    }
    const unsigned lds_addr = (unsigned)(size_t)(__attribute__((address_space(3))) float *)(&lds[0]) + (threadIdx.x & 255) * 16;
    int k = 0;
    STREAM(k++, REGS1, "");
    STREAM(k++, REGS1, "v_fma_f32 v\\r, v30, v31, v32");
    STREAM(k++, REGS1, "v_fma_f32 v10, v10, v31, v32");
    STREAM(k++, REGS1, "v_mul_f32 v\\r, v30, v31");
    STREAM(k++, REGS1, "v_mov_b32 v\\r, v30");
    STREAM(k++, REGS1, "v_fmac_f32_dpp v\\r, v30, v31 row_ror:1 row_mask:0xf bank_mask:0xf");
    STREAM(k++, REGS1, "v_fmac_f32_dpp v10, v30, v31 row_ror:1 row_mask:0xf bank_mask:0xf");
    STREAM(k++, REGS1, "v_mov_b32_dpp v\\r, v30 row_ror:1 row_mask:0xf bank_mask:0xf");
    STREAM(k++, REGS1, "v_mov_b32_dpp v10, v10 row_ror:1 row_mask:0xf bank_mask:0xf\n s_nop 1");
    STREAM(k++, REGS1, "v_add_f32_dpp v\\r, v30, v31 row_ror:8 row_mask:0xf bank_mask:0xf");
    STREAM(k++, REGS1, "v_add_f32_dpp v10, v30, v10 row_ror:8 row_mask:0xf bank_mask:0xf");
    STREAM(k++, REGS2, "v_pk_mul_f32 v[\\r:\\r+1], v[30:31], v[32:33]");
    STREAM(k++, REGS2, "v_pk_mul_f32 v[10:11], v[10:11], v[30:31]");
    STREAM(k++, REGS2, "v_pk_add_f32 v[\\r:\\r+1], v[30:31], v[32:33]");
    STREAM(k++, REGS2, "v_pk_add_f32 v[10:11], v[10:11], v[30:31]");
    STREAM(k++, REGS2, "v_pk_fma_f32 v[\\r:\\r+1], v[30:31], v[32:33], v[34:35]");
    STREAM(k++, REGS2, "v_pk_fma_f32 v[10:11], v[10:11], v[32:33], v[34:35]");
    STREAM(k++, REGS1, "v_exp_f32 v\\r, v30");
    STREAM(k++, REGS1, "v_exp_f32 v10, v10");
    STREAM(k++, REGS1, "v_rcp_f32 v\\r, v30");
    STREAM(k++, REGS1, "v_rcp_f32 v10, v10");
    STREAM(k++, REGS1, "v_exp_f32 v10, v11\n s_nop 0\n v_add_f32 v11, v10, v31");
    STREAM(k++, REGS2, "v_permlane16_swap_b32 v\\r, v[\\r+1]");
    STREAM(k++, REGS2, "v_permlane16_swap_b32 v10, v11\n s_nop 1");
    STREAM(k++, REGS2, "v_permlane32_swap_b32 v\\r, v[\\r+1]");
    STREAM(k++, REGS2, "v_permlane32_swap_b32 v10, v11\n s_nop 1");
    STREAM(k++, REGS1, "v_bfi_b32 v\\r, v37, v31, v32");
    STREAM(k++, REGS1, "v_bfi_b32 v10, v37, v10, v32");
    STREAM(k++, REGS1, "v_cndmask_b32_e64 v\\r, v30, v31, s[20:21]");
    STREAM(k++, REGS1, "v_cndmask_b32_e64 v10, v10, v31, s[20:21]");
    STREAM(k++, REGS2, "v_cvt_f64_f32 v[\\r:\\r+1], v30");
    STREAM(k++, REGS2, "v_cvt_f64_f32 v[10:11], v10");
    STREAM(k++, REGS2, "v_cvt_f32_f64 v\\r, v[30:31]");
    STREAM(k++, REGS2, "v_fma_f64 v[\\r:\\r+1], v[30:31], v[32:33], v[34:35]");
    STREAM(k++, REGS2, "v_fma_f64 v[10:11], v[10:11], v[32:33], v[34:35]");
    STREAM(k++, REGS2, "v_cmp_gt_f64 vcc, v[30:31], v[32:33]");
    STREAM(k++, REGS2, "v_cmp_gt_f64 vcc, v[10:11], v[32:33]\n v_cndmask_b32_e32 v10, v30, v31, vcc");
    STREAM(k++, REGS1, "v_cmp_gt_f32 vcc, v30, v31");
    STREAM(k++, REGS1, "v_cmp_class_f32 vcc, v30, v37");
    STREAM(k++, REGS1, "v_cmp_class_f32 vcc, v10, v37\n v_cndmask_b32_e32 v10, v30, v31, vcc");
    STREAM(k++, REGS1, "v_max3_f32 v\\r, |v30|, |v31|, |v32|");
    STREAM(k++, REGS1, "v_max3_f32 v10, |v10|, |v31|, |v32|");
    STREAM(k++, REGS1, "v_add3_u32 v\\r, v30, v31, v32");
    STREAM(k++, REGS1, "v_add3_u32 v10, v10, v31, v32");
    STREAM(k++, REGS1, "s_nop 0");
    STREAM(k++, REGS1, "s_nop 1");
    STREAM(k++, SREGS, "s_add_u32 s\\r, s20, 1");
    STREAM(k++, SREGS, "s_add_u32 s22, s22, 1");
    STREAM(k++, REGS2, "s_and_b64 s[22:23], s[20:21], exec");
    STREAM(k++, REGS2, "ds_read_b128 v[12:15], v40\n s_waitcnt lgkmcnt(0)");
    STREAM(k++, REGS2, "ds_read_b128 v[10:13], v40\n ds_read_b128 v[14:17], v40\n ds_read_b128 v[18:21], v40\n ds_read_b128 v[22:25], v40\n s_waitcnt lgkmcnt(0)");
    STREAM(k++, REGS2, "v_fma_f32 v\\r, v30, v31, v32\n v_fma_f32 v[\\r+1], v33, v34, v35");
    STREAM(k++, REGS2, "v_mul_f32 v10, v10, v30\n v_mul_f32 v11, v11, v31");
    if (lane == 0) {
        cyc[(2 * NKIND_MAX) * 5 + pass * 5 + wave] = (unsigned long long)k;
        __threadfence_block();
        atomicAdd((int *)&done, 1);
    }
}

int main() {
    static_assert(sizeof(KINDS) / sizeof(KINDS[0]) <= NKIND_MAX, "table");
    const size_t ncyc = (2 * NKIND_MAX + 2) * 5;
    unsigned long long *dc; unsigned *ds; float *df;
    if (hipMalloc(&dc, ncyc * sizeof(*dc)) != hipSuccess || hipMalloc(&ds, 10 * sizeof(*ds)) != hipSuccess || hipMalloc(&df, 320 * sizeof(*df)) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); return 1; }
    std::vector<unsigned long long> c(ncyc);
    unsigned simd[10];
    // each pass runs twice, the second run is kept (instruction cache, clocks)
    for (int rep = 0; rep < 2; ++rep) {
        hipMemset(dc, 0, ncyc * sizeof(*dc));
        hipMemset(ds, 0xff, sizeof(simd));
        hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(256), 0, 0, dc, ds, df, 0);
        if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "pass 0 failed\n"); return 1; }
        hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(320), 0, 0, dc, ds, df, 1);
        if (hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "pass 1 failed\n"); return 1; }
    }
    hipMemcpy(c.data(), dc, ncyc * sizeof(*dc), hipMemcpyDeviceToHost);
    hipMemcpy(simd, ds, sizeof(simd), hipMemcpyDeviceToHost);
    for (int pass = 0; pass < 2; ++pass)
        for (int w = 0; w < 4; ++w)
            if ((int)c[(2 * NKIND_MAX) * 5 + pass * 5 + w] != NKIND) { fprintf(stderr, "pass %d wave %d ran %d streams, the table has %d\n", pass, w, (int)c[(2 * NKIND_MAX) * 5 + pass * 5 + w], NKIND); return 1; }
    printf("# tools/solo_issue_probe.hip on one MI355X: s_memtime cycles per instruction of a lone wave, one workgroup, waves 0..3 one per SIMD.\n");
    printf("# A stream is %d passes over %d .irp steps of the instruction(s) named; the empty loop's cycles are subtracted; 'per instr' divides by\n", ITERS, BODY);
    printf("# the instructions of a step (a pair with its pad counts as 2).  indep: eight rotating destinations; dep: each reads the one before.\n");
    for (int pass = 0; pass < 2; ++pass) {
        printf("\n# pass %d: %s\n", pass, pass ? "a fifth wave runs a plain v_fma_f32 stream beside them (HW_ID SIMD of waves 0..4 below; the wave that shares its SIMD pays)" : "four waves alone");
        printf("# HW_ID.SIMD_ID of waves:");
        for (int w = 0; w < (pass ? 5 : 4); ++w) printf(" %u", simd[pass * 5 + w]);
        printf("\n# %-44s %8s %8s %8s %8s   %s\n", "kind", "wave0", "wave1", "wave2", "wave3", "per step, wave 1 (cycles)");
        for (int k = 0; k < NKIND; ++k) {
            printf("%-46s", KINDS[k].name);
            double step1 = 0;
            for (int w = 0; w < 4; ++w) {
                const double t = (double)c[(pass * NKIND + k) * 5 + w], t0 = (double)c[(pass * NKIND + 0) * 5 + w];
                if (k == 0) { printf(" %8.1f", t / ITERS); continue; }
                const double per_step = (t - t0) / (double)(ITERS * BODY);
                if (w == 1) step1 = per_step;
                printf(" %8.2f", per_step / KINDS[k].per);
            }
            if (k == 0) printf("   (cycles per pass, with the two stamps)\n");
            else printf("   %6.2f  %s\n", step1, KINDS[k].note);
        }
    }
    return 0;
}
