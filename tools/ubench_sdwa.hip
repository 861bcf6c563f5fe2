// What does v_add_u32_sdwa cost to issue on gfx950?  The coarse screen's level image keeps four byte scores of a
// lane in one dword and lets the cell's addition pick its byte (src0_sel:BYTE_n), and takes a 16-bit half of the level pair the
// same way (src0_sel:WORD_1): that only pays if the SDWA form issues like the plain addition (~2.4 SIMD cycles) and not like the
// v_max3_f32 / v_med3_i32 class (~4.7).  Same loop as tools/ubench_operands.hip, at 4 and 6 waves per SIMD; the alternative layout
// (plain ds_read_u8 with immediate offsets, no select) is timed beside it.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench_sdwa.hip -o /tmp/ubench_sdwa && /tmp/ubench_sdwa
#include <hip/hip_runtime.h>
#include <cstdio>

#define CLOBBER "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71"
#define INIT asm volatile("v_mov_b32 v40, 1.0\n v_mov_b32 v41, 2.0\n v_mov_b32 v42, 0.5\n v_mov_b32 v43, 4.0\n v_mov_b32 v44, 1.0\n v_mov_b32 v45, 2.0\n v_mov_b32 v46, 0.5\n v_mov_b32 v47, 4.0\n" \
                          "v_mov_b32 v48, 1.0\n v_mov_b32 v49, 2.0\n v_mov_b32 v50, 0.5\n v_mov_b32 v51, 4.0\n v_mov_b32 v52, 1.0\n v_mov_b32 v53, 2.0\n v_mov_b32 v54, 0.5\n v_mov_b32 v55, 4.0\n" \
                          "v_mov_b32 v56, 1.0\n v_mov_b32 v57, 2.0\n v_mov_b32 v58, 0.5\n v_mov_b32 v59, 4.0\n v_mov_b32 v60, 1.0\n v_mov_b32 v61, 2.0\n v_mov_b32 v62, 0.5\n v_mov_b32 v63, 4.0\n" \
                          "v_mov_b32 v64, 1.0\n v_mov_b32 v65, 2.0\n v_mov_b32 v66, 0.5\n v_mov_b32 v67, 4.0\n v_mov_b32 v68, 1.0\n v_mov_b32 v69, 2.0\n v_mov_b32 v70, 0.5\n v_mov_b32 v71, 4.0" ::: CLOBBER)
#define SDWA(sel) " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" sel " src1_sel:DWORD\n"

template <int MODE> __global__ void k_rate(unsigned* out, int iters)
{
    __shared__ unsigned lds[1024];
    for (int i = threadIdx.x; i < 1024; i += blockDim.x) lds[i] = i;
    __syncthreads();
    const unsigned addr = (unsigned)(size_t)lds + (threadIdx.x & 63) * 4;      // lane l reads its own dword: no bank conflicts
    INIT;
    for (int i = 0; i < iters; i++) {
        if (MODE == 0)          // plain v_add_u32 (the full-rate reference)
            asm volatile("v_add_u32 v64, v41, v42\n v_add_u32 v65, v42, v43\n v_add_u32 v66, v43, v44\n v_add_u32 v67, v44, v45\n"
                         "v_add_u32 v68, v45, v46\n v_add_u32 v69, v46, v47\n v_add_u32 v70, v47, v48\n v_add_u32 v71, v48, v49" ::: CLOBBER);
        else if (MODE == 1)     // SDWA, byte selects 0 .. 3 on src0
            asm volatile("v_add_u32_sdwa v64, v41, v42" SDWA("BYTE_0") "v_add_u32_sdwa v65, v42, v43" SDWA("BYTE_1") "v_add_u32_sdwa v66, v43, v44" SDWA("BYTE_2") "v_add_u32_sdwa v67, v44, v45" SDWA("BYTE_3")
                         "v_add_u32_sdwa v68, v45, v46" SDWA("BYTE_0") "v_add_u32_sdwa v69, v46, v47" SDWA("BYTE_1") "v_add_u32_sdwa v70, v47, v48" SDWA("BYTE_2") "v_add_u32_sdwa v71, v48, v49" SDWA("BYTE_3") ::: CLOBBER);
        else if (MODE == 2)     // SDWA, word selects on src0
            asm volatile("v_add_u32_sdwa v64, v41, v42" SDWA("WORD_0") "v_add_u32_sdwa v65, v42, v43" SDWA("WORD_1") "v_add_u32_sdwa v66, v43, v44" SDWA("WORD_0") "v_add_u32_sdwa v67, v44, v45" SDWA("WORD_1")
                         "v_add_u32_sdwa v68, v45, v46" SDWA("WORD_0") "v_add_u32_sdwa v69, v46, v47" SDWA("WORD_1") "v_add_u32_sdwa v70, v47, v48" SDWA("WORD_0") "v_add_u32_sdwa v71, v48, v49" SDWA("WORD_1") ::: CLOBBER);
        else if (MODE == 3)     // v_med3_i32 (what the look-up's clamp costs today)
            asm volatile("v_med3_i32 v64, v41, v42, v43\n v_med3_i32 v65, v42, v43, v44\n v_med3_i32 v66, v43, v44, v45\n v_med3_i32 v67, v44, v45, v46\n"
                         "v_med3_i32 v68, v45, v46, v47\n v_med3_i32 v69, v46, v47, v48\n v_med3_i32 v70, v47, v48, v49\n v_med3_i32 v71, v48, v49, v50" ::: CLOBBER);
        else if (MODE == 4)     // the screen's cell as it is: v_add_u32 then v_max3_f32
            asm volatile("v_add_u32 v64, v41, v42\n v_max3_f32 v56, v64, v43, v57\n v_add_u32 v65, v42, v43\n v_max3_f32 v57, v65, v44, v58\n"
                         "v_add_u32 v66, v43, v44\n v_max3_f32 v58, v66, v45, v59\n v_add_u32 v67, v44, v45\n v_max3_f32 v59, v67, v46, v56" ::: CLOBBER);
        else if (MODE == 5)     // the cell with the byte select folded into its addition
            asm volatile("v_add_u32_sdwa v64, v41, v42" SDWA("BYTE_0") "v_max3_f32 v56, v64, v43, v57\n v_add_u32_sdwa v65, v41, v43" SDWA("BYTE_1") "v_max3_f32 v57, v65, v44, v58\n"
                         "v_add_u32_sdwa v66, v41, v44" SDWA("BYTE_2") "v_max3_f32 v58, v66, v45, v59\n v_add_u32_sdwa v67, v41, v45" SDWA("BYTE_3") "v_max3_f32 v59, v67, v46, v56" ::: CLOBBER);
        else if (MODE == 6)     // v_bfe_u32 (an explicit byte extract, if the select had to be its own instruction)
            asm volatile("v_bfe_u32 v64, v41, 8, 8\n v_bfe_u32 v65, v42, 16, 8\n v_bfe_u32 v66, v43, 8, 8\n v_bfe_u32 v67, v44, 16, 8\n"
                         "v_bfe_u32 v68, v45, 8, 8\n v_bfe_u32 v69, v46, 16, 8\n v_bfe_u32 v70, v47, 8, 8\n v_bfe_u32 v71, v48, 16, 8" ::: CLOBBER);
        else if (MODE == 7)     // the alternative layout: eight plain ds_read_u8 off one address, immediate offsets
            asm volatile("ds_read_u8 v64, %0\n ds_read_u8 v65, %0 offset:1\n ds_read_u8 v66, %0 offset:2\n ds_read_u8 v67, %0 offset:3\n"
                         "ds_read_u8 v68, %0 offset:256\n ds_read_u8 v69, %0 offset:257\n ds_read_u8 v70, %0 offset:258\n ds_read_u8 v71, %0 offset:259\n s_waitcnt lgkmcnt(0)" :: "v"(addr) : CLOBBER);
        else if (MODE == 8)     // ... against two ds_read_b32 for the same eight scores
            asm volatile("ds_read_b32 v64, %0\n ds_read_b32 v68, %0 offset:256\n s_waitcnt lgkmcnt(0)" :: "v"(addr) : CLOBBER);
    }
    unsigned r;
    asm volatile("v_add_u32 %0, v64, v71\n v_add_u32 %0, %0, v56" : "=v"(r) :: CLOBBER);
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

template <int MODE> void run(const char* name, int waves_per_simd, int per_iter)
{
    unsigned* d; (void)hipMalloc(&d, 256 * 4 * 8 * 64 * 4);
    const int iters = 100000;
    dim3 grid(256 * waves_per_simd), block(256);
    hipEvent_t a, b; (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    k_rate<MODE><<<grid, block>>>(d, 1000); (void)hipDeviceSynchronize();
    (void)hipEventRecord(a); k_rate<MODE><<<grid, block>>>(d, iters); (void)hipEventRecord(b); (void)hipEventSynchronize(b);
    float ms; (void)hipEventElapsedTime(&ms, a, b);
    const double cyc = ms * 1e-3 * 2.4e9;
    printf("%-62s waves/simd=%d  %.3f ms  -> %.2f cycles(@2.4GHz) per wave-instruction and SIMD\n", name, waves_per_simd, ms, cyc / ((double)iters * per_iter * waves_per_simd));
    (void)hipFree(d);
}

int main()
{
    for (int w : {4, 6}) {
        run<0>("v_add_u32", w, 8);
        run<1>("v_add_u32_sdwa src0_sel:BYTE_0..3", w, 8);
        run<2>("v_add_u32_sdwa src0_sel:WORD_0/1", w, 8);
        run<3>("v_med3_i32", w, 8);
        run<6>("v_bfe_u32", w, 8);
        run<4>("screen cell: v_add_u32 + v_max3_f32", w, 8);
        run<5>("screen cell: v_add_u32_sdwa BYTE_n + v_max3_f32", w, 8);
        run<7>("8 x ds_read_u8, immediate offsets (per read)", w, 8);
        run<8>("2 x ds_read_b32 (per read)", w, 2);
    }
    return 0;
}
