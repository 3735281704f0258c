// k_haar_select_hop.hip -- the generic stage 2 with frames at a row hop (frame phases): k_haar_select.hip
// compiled a second time as haar_select_hop_kernel (see k_haar_select32_hop.hip).
#define LBAD_STAGE2_HOP 1
#include "k_haar_select.hip"
