// k_haar_select32_hop.hip -- the specialised stage 2 with frames at a row hop (frame phases): the kernels of
// k_haar_select32.hip compiled a second time as haar_select32_hop_kernel, in a translation unit of their own so that the
// instances the batch path launches keep their code, their names and their file.
#define LBAD_STAGE2_HOP 1
#include "k_haar_select32.hip"
