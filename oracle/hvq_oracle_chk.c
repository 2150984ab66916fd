/* oracle/hvq_oracle_chk.c -- TEST INFRASTRUCTURE ONLY: the checked mode of the oracle, i.e. hvq_oracle.c compiled a second time
 * with every input-controlled access behind a guard (see the comment at the head of that file). */
#define HVQO_CHECKED 1
#include "hvq_oracle.c"
